/* Groth16 proof verification of batches on an MI355X (what snarkjs `groth16 verify` does), with the BN254 optimal ate pairing.
 *
 * Verifying key: nPublic; alpha1 (G1), beta2, gamma2, delta2 (G2); IC[0 .. nPublic] (G1).
 *
 * Pairing: BN254's optimal ate pairing e(P, Q), P in G1 (y^2 = x^3 + 3 over Fq), Q in G2 on the twist y^2 = x^3 + 3 / (9 + u)
 * over Fq2 = Fq[u]/(u^2 + 1): the Miller loop of length 6x + 2 (x = 4965661367192848881) with the two final lines at pi(Q)
 * and -pi^2(Q), then the final exponent (q^12 - 1) / r exactly (not a multiple of it).  Tower: Fq6 = Fq2[v]/(v^3 - (9 + u)),
 * Fq12 = Fq6[w]/(w^2 - v).  A GT element is GWB_GT_BYTES = 384 bytes: 12 canonical 32-byte little-endian Fq values in the
 * order c0.b0.a0, c0.b0.a1, c0.b1.a0, c0.b1.a1, c0.b2.a0, c0.b2.a1, c1.b0.a0, ..., c1.b2.a1 (snarkjs's vk_alphabeta_12 nesting).
 *
 * Points are canonical little-endian bytes: G1 x, y (64 B); G2 x.c0, x.c1, y.c0, y.c1 (128 B); all zero = the point at infinity.
 *
 * Per-row verification.  A row is one proof in the prover's layout (GWB_GROTH16_PROOF_BYTES = 256: A, B, C) and nPublic
 * canonical 32-byte public signals.  Its uint32 status is set by the first rule that applies:
 *   GWB_G16V_PUBLIC    a public signal >= r (signals are not reduced; snarkjs's publicInputsAreValid)
 *   GWB_G16V_POINT     a coordinate >= q, or A, B or C neither infinity nor on its curve
 *   GWB_G16V_SUBGROUP  B not in G2's order-r subgroup (G1's cofactor is 1: A and C need no check)
 *   GWB_G16V_EQUATION  e(A, B) != e(alpha1, beta2) e(vk_x, gamma2) e(C, delta2),  vk_x = IC_0 + sum_i s_i IC_i
 *   GWB_G16V_VALID     none of the above (0)
 * Infinity is allowed for A, B and C; the equation then decides.
 *
 * The key loader refuses, with a message: a coordinate >= q, a point off its curve, a G2 key point outside the order-r
 * subgroup (checked once, on the host) and a point count that does not match nPublic.  The key's device data (the line
 * coefficients of gamma2 and delta2, e(alpha1, beta2), the IC tables) are made on the device that is current at the first
 * verify or alphabeta call and stay there.  Return and status conventions are those of graph_witness_r1cs.h (0 on success,
 * 1 on failure with status filled).  Verify calls on one key share its workspace: enqueue them on one stream.  A key may be
 * used from one thread at a time. */
#ifndef CWC_AMD_GRAPH_WITNESS_GROTH16_VERIFY_H
#define CWC_AMD_GRAPH_WITNESS_GROTH16_VERIFY_H

#include <stddef.h>
#include <stdint.h>

#include "graph_witness_groth16.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gwb_g16vk gwb_g16vk_t;

#define GWB_GT_BYTES 384
#define GWB_G16V_VALID 0u
#define GWB_G16V_PUBLIC 1u
#define GWB_G16V_POINT 2u
#define GWB_G16V_SUBGROUP 3u
#define GWB_G16V_EQUATION 4u

typedef struct {
  uint32_t n_public;
} gwb_g16vk_info_t;

/* The key of a loaded .zkey (its Montgomery "LEM" points converted). */
int gwb_g16vk_from_zkey(const gwb_zkey_t *z, gwb_g16vk_t **out, gw_status_t *status);
/* Raw canonical points: alpha1 (64 B), beta2, gamma2, delta2 (128 B each), then IC (64 B each); len must be
 * 448 + 64 (n_public + 1). */
int gwb_g16vk_load(const void *points, size_t len, uint32_t n_public, gwb_g16vk_t **out, gw_status_t *status);
int gwb_g16vk_info(const gwb_g16vk_t *vk, gwb_g16vk_info_t *info);
/* The key's points back, in gwb_g16vk_load's layout; len must be 448 + 64 (nPublic + 1). */
int gwb_g16vk_points(const gwb_g16vk_t *vk, void *out, size_t len);
/* e(alpha1, beta2), GWB_GT_BYTES; computed on the current device at the first call (synchronous). */
int gwb_g16vk_alphabeta(gwb_g16vk_t *vk, void *gt, gw_status_t *status);
void gwb_g16vk_free(gwb_g16vk_t *vk);

/* Device proofs [batch][256 B], device public signals [batch][n_public][32 B] (n_public must be the key's) -> device
 * d_status [batch] uint32.  Asynchronous on hip_stream with the ordering contract of gwb_groth16_prove_batch_device. */
int gwb_groth16_verify_batch_device(gwb_g16vk_t *vk, const void *d_proofs, const void *d_public, size_t n_public, size_t batch,
                                    void *d_status, void *hip_stream, gw_status_t *status);
/* The same with host arrays; synchronous. */
int gwb_groth16_verify_batch_host(gwb_g16vk_t *vk, const void *proofs, const void *pub, size_t n_public, size_t batch,
                                  void *status_out, gw_status_t *status);
/* Measurement and test aid: d_gt[i] = e(d_g1[i], d_g2[i]) (GWB_GT_BYTES each) for n device pairs (64 B and 128 B canonical;
 * the points are not validated: they must lie on their curves, in G1 and G2), by the general path with a changing Q.
 * Asynchronous on hip_stream (its workspace is allocated and freed in stream order). */
int gwb_bn254_pairing_batch_device(const void *d_g1, const void *d_g2, size_t n, void *d_gt, void *hip_stream, gw_status_t *status);
/* Measurement and test aid, and what gwb_zkey_check_g2 and gwb_ptau_check_g2 run: d_status[i] (uint32) for n device G2 points
 * (128 B each: x.c0, x.c1, y.c0, y.c1 in form GWB_FORM_CANONICAL or GWB_FORM_MONTGOMERY) is
 *   GWB_G16V_VALID     the point is in G2's order-r subgroup (infinity, all zero bytes, included)
 *   GWB_G16V_POINT     a coordinate >= q, or the point is not on the twist
 *   GWB_G16V_SUBGROUP  on the twist, outside the subgroup
 * method 0 decides by [x + 1] P + psi([x] P) + psi^2([x] P) = psi^3([2x] P) (x the BN parameter, psi the untwist-Frobenius-twist
 * endomorphism; r1cs/g2_subgroup_gfx950.hpp), method 1 by [r] P = O, the verifier's rule (cross-check and baseline).  An unknown
 * form or method returns 1 before any device work; n = 0 does nothing.  Asynchronous on hip_stream. */
int gwb_bn254_g2_check_batch_device(const void *d_points, size_t n, uint32_t form, uint32_t method, void *d_status, void *hip_stream,
                                    gw_status_t *status);

#ifdef __cplusplus
}
#endif
#endif /* CWC_AMD_GRAPH_WITNESS_GROTH16_VERIFY_H */
