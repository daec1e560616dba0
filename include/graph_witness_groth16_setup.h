/* Groth16 proving keys on an MI355X from a circuit's `.r1cs`: the circuit-specific setup (arkworks'
 * generate_random_parameters / circuit_specific_setup; the single-party equivalent of snarkjs `groth16 setup`).
 *
 * TRUST.  Whoever knows the trapdoor (tau, alpha, beta, gamma, delta) can forge proofs for the key.  This is a single-party
 * setup for development, tests and deployments where the key's maker is trusted; it is not an MPC ceremony.  A drawn trapdoor
 * is discarded (zeroed on the host and on the device) before the call returns.
 *
 * Definition.  The R1CS has nC constraints (A_k, B_k, C_k), nW wires and nPub = nPubOut + nPubIn public signals; n = 2^p is
 * the QAP domain that gwb_r1cs_qap_info reports, w that domain's generator and g the 2n-th root used by the witness map
 * (graph_witness_r1cs.h); the trapdoor values lie in [1, r).
 *   Lagrange values at tau, on the n domain:                    L_k = (tau^n - 1) / n * w^k / (tau - w^k)
 *   and on the odd points of the 2n domain:                     M_j = (tau^2n - 1) / 2n * g w^j / (tau - g w^j)
 *   per wire i:  u_i = sum_k A_k[i] L_k  (+ L_{nC+i} for i <= nPub: the public rows of the witness map),
 *                v_i = sum_k B_k[i] L_k,   w_i = sum_k C_k[i] L_k
 *   section 5 (A):   A_i  = u_i G1                 section 6 (B1):  B1_i = v_i G1         section 7 (B2):  B2_i = v_i G2
 *   section 3 (IC):  IC_i = ((beta u_i + alpha v_i + w_i) / gamma) G1                     for i <= nPub
 *   section 8 (C):   C_{i-nPub-1} = ((beta u_i + alpha v_i + w_i) / delta) G1             for i > nPub
 *   section 9 (H):   H_j  = (M_j / delta) G1
 *   header:          alpha G1, beta G1, beta G2, gamma G2, delta G1, delta G2
 * G1 = (1, 2) and G2 are the generators snarkjs uses.  A scalar of 0 gives the point at infinity, stored as all-zero bytes.
 * With this key the proofs of graph_witness_groth16.h satisfy the equation of graph_witness_groth16_verify.h.
 *
 * Output: a complete iden3 binfile "zkey" v1 (the layout in graph_witness_groth16.h / r1cs/zkey.cc), accepted by
 * gwb_zkey_load, sections 1 to 10 in ascending order.  Two caveats about the format:
 *   section 10 holds 64 zero bytes (no circuit hash) and u32 0 (no contributions);
 *   section 4 holds the coefficients as snarkjs `zkey new` lays them out: per constraint in file order first its A terms
 *   (0, k, signal, value), then its B terms (1, k, signal, value), in the order the `.r1cs` stores them, then
 *   (0, nC + s, s, 1) for s = 0 .. nPub; each value is stored as value * R^2 mod r (R = 2^256), canonical little-endian.
 *   This layout is restated from snarkjs's writer and, like the loader's reading of it, has not been cross-checked against
 *   snarkjs itself (no snarkjs output is available to this project).  The prover here does not read section 4.
 *
 * Return and status conventions are those of graph_witness_r1cs.h (0 on success, 1 on failure with status filled).  The call
 * is synchronous and runs on the current device.  Every device buffer that held the trapdoor's powers, the Lagrange values,
 * u, v, w or the key scalars is zeroed before it is released, on every error path too. */
#ifndef CWC_AMD_GRAPH_WITNESS_GROTH16_SETUP_H
#define CWC_AMD_GRAPH_WITNESS_GROTH16_SETUP_H

#include <stddef.h>
#include <stdint.h>

#include "graph_witness_groth16.h"

#ifdef __cplusplus
extern "C" {
#endif

/* canonical little-endian values, each in [1, r) */
typedef struct {
  uint8_t tau[32], alpha[32], beta[32], gamma[32], delta[32];
} gwb_groth16_trapdoor_t;

/* trapdoor == NULL: each value is drawn uniformly from [1, r) (the prover's rejection sampler over getrandom()), tau again
 * while tau^2n = 1.  A supplied trapdoor is refused with a message, on the host and before the device is touched, when a
 * value is 0 or >= r, or when tau^2n = 1 (tau on either domain; tau = r - 1 is the smallest example).  A domain above 2^27
 * and custom-gate files are refused by the handle.  *zkey is released with gwb_groth16_setup_free. */
int gwb_groth16_setup(gwb_r1cs_t *r, const gwb_groth16_trapdoor_t *trapdoor, void **zkey, size_t *zkey_len,
                      gw_status_t *status);
void gwb_groth16_setup_free(void *zkey);

/* Measurement and test aid, like gwb_bn254_pairing_batch_device: d_scalars [n][32 B] canonical little-endian (values >= r
 * are reduced) -> d_points [n][64 B] (group 1) or [n][128 B] (group 2), k_i times the generator, canonical little-endian
 * affine coordinates, infinity = zero bytes.  Asynchronous on hip_stream (its workspace is allocated and freed in stream
 * order; the table of generator multiples is built at the first call of a process on a device, synchronously). */
int gwb_bn254_gen_mul_batch_device(const void *d_scalars, size_t n, uint32_t group, void *d_points, void *hip_stream,
                                   gw_status_t *status);

/* ms[5] of the last gwb_groth16_setup call of the process (HIP events): Lagrange values, column sums, key scalars, G1
 * multiplications, G2 multiplications and both conversions to affine.  1 when no call has completed yet. */
int gwb_groth16_setup_phase_ms(float *ms);

#ifdef __cplusplus
}
#endif
#endif /* CWC_AMD_GRAPH_WITNESS_GROTH16_SETUP_H */
