/* Groth16 proofs of witness batches on an MI355X, from a circuit's `.zkey` and `.r1cs` (what snarkjs `groth16 prove` does).
 *
 * For a witness row w (wire 0 = 1, nVars wires), nPub = nPubOut + nPubIn, two scalars r, s in [0, r) and the row's witness
 * map h (gwb_r1cs_qap_*, natural order, n = domainSize elements):
 *   pi_A = alpha1 + sum_{i<nVars} w_i A_i + r delta1                                                        (G1)
 *   pi_B = beta2  + sum_{i<nVars} w_i B2_i + s delta2                                                       (G2)
 *   B1   = beta1  + sum_{i<nVars} w_i B1_i + s delta1                                                       (G1)
 *   pi_C = sum_{i=nPub+1}^{nVars-1} w_i C_{i-nPub-1} + sum_{j<n} h_j H_j + s pi_A + r B1 - (r s) delta1     (G1)
 * Output per row: GWB_GROTH16_PROOF_BYTES = 256 bytes, the affine coordinates A.x, A.y, B.x.c0, B.x.c1, B.y.c0, B.y.c1, C.x,
 * C.y as 32-byte canonical little-endian integers (Fq2 = Fq[u]/(u^2 + 1), x = x.c0 + x.c1 u); the point at infinity is all
 * zero bytes.
 *
 * The `.zkey` (iden3 binfile "zkey" v1, Groth16) is validated when loaded: BN254's q and r, section sizes against its header,
 * coordinates below q, every point other than infinity on its curve.  G2 points are not checked for subgroup membership.
 * The prover takes the witness map from the `.r1cs` handle (section 4 of the zkey is bounds-checked only), so the two files
 * must agree: zkey nVars == r1cs nWires, nPublic == nPubOut + nPubIn, domainSize == the QAP domain size; otherwise the
 * call is refused.
 *
 * Return and status conventions are those of graph_witness_r1cs.h (0 on success, 1 on failure with status filled).  The
 * curve points are uploaded to the device that is current at the first prove call and stay there; the device workspace
 * belongs to the zkey handle, grows on demand and is released by gwb_zkey_free.  A batch whose workspace would exceed
 * CWC_GROTH16_WORKSPACE_MB (read once per process, default 4096) runs in sub-batches.  Prove calls on one handle share
 * its workspace: enqueue them on one stream.  A handle may be used from one thread at a time. */
#ifndef CWC_AMD_GRAPH_WITNESS_GROTH16_H
#define CWC_AMD_GRAPH_WITNESS_GROTH16_H

#include <stddef.h>
#include <stdint.h>

#include "graph_witness_r1cs.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gwb_zkey gwb_zkey_t;

typedef struct {
  uint32_t n_vars, n_public, domain_size;
  uint64_t n_coefs;
} gwb_zkey_info_t;

#define GWB_GROTH16_PROOF_BYTES 256

int gwb_zkey_load(const void *data, size_t len, gwb_zkey_t **out, gw_status_t *status);
void gwb_zkey_free(gwb_zkey_t *z);
int gwb_zkey_info(const gwb_zkey_t *z, gwb_zkey_info_t *info);

/* Device rows [batch][n_witness][32 B] in form_in (GWB_FORM_CANONICAL or GWB_FORM_MONTGOMERY; n_witness == nVars; elements
 * >= r are reduced mod r) -> d_proofs [batch][256 B].  rs: host array [batch][2][32 B] of canonical r, s (each below r), or
 * NULL: drawn uniformly from [0, r) by rejection sampling from getrandom().  Asynchronous on hip_stream with the ordering
 * contract of gwb_r1cs_check_batch_device; rs is read before the call returns. */
int gwb_groth16_prove_batch_device(gwb_zkey_t *z, gwb_r1cs_t *r, const void *d_witness, size_t n_witness, size_t batch,
                                   uint32_t form_in, const void *rs, void *d_proofs, void *hip_stream, gw_status_t *status);
/* The same with host rows (canonical) and host proofs; synchronous. */
int gwb_groth16_prove_batch_host(gwb_zkey_t *z, gwb_r1cs_t *r, const void *witness, size_t n_witness, size_t batch,
                                 const void *rs, void *proofs, gw_status_t *status);
/* One `.wtns` image, validated as gwb_r1cs_check_wtns validates it -> proof [256 B]; rs is [2][32 B] or NULL. */
int gwb_groth16_prove_wtns(gwb_zkey_t *z, gwb_r1cs_t *r, const void *wtns, size_t wtns_len, const void *rs, void *proof,
                           gw_status_t *status);
/* Measurement aid (as gwb_r1cs_qap_time_phases): with on != 0, later prove calls record HIP events around their phases (for
 * the last sub-batch of a call); gwb_groth16_phase_ms waits for the last call and writes ms[5] = witness map, scalar
 * preparation and sort, G1 MSMs (A, B1, C, H), G2 MSM (B2), assembly. */
int gwb_groth16_time_phases(gwb_zkey_t *z, int on);
int gwb_groth16_phase_ms(gwb_zkey_t *z, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* CWC_AMD_GRAPH_WITNESS_GROTH16_H */
