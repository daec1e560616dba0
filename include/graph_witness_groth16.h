/* Groth16 proofs of witness batches on an MI355X, from a circuit's `.zkey` alone or with its `.r1cs` (what snarkjs `groth16
 * prove` does).
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
 * coordinates below q, every point other than infinity on its curve.  G2 points are not checked for subgroup membership by
 * the loader; gwb_zkey_check_g2 checks them on the device when asked.
 * Section 4 (the coefficients) is bounds-checked at load: matrix 0 or 1, constraint < domainSize, signal < nVars.
 *
 * The witness map h comes from one of two places.  With an `.r1cs` handle the prover takes it from there, as before, and the
 * two files must agree: zkey nVars == r1cs nWires, nPublic == nPubOut + nPubIn, domainSize == the QAP domain size; otherwise
 * the call is refused.  Sizes are all that is compared there: gwb_zkey_check_r1cs compares the coefficients.  With r == NULL
 * the map comes from the zkey's own section 4, which is what snarkjs and rapidsnark do.  An entry (matrix m, constraint c,
 * signal s, value v) adds (v / R^2) w_s, R = 2^256, to a_c (m = 0) or b_c (m = 1), and c_i = a_i b_i for every row (snarkjs
 * buildABC1); the public rows are entries like any other (snarkjs `zkey new` writes (0, nC + i, i, R^2 mod r) for i = 0 ..
 * nPublic).  Entries may come in any order, entries with the same (m, c, s) add up, a zero value contributes nothing and a row
 * without entries is zero; the domain, roots and output are those of graph_witness_r1cs.h with n = domainSize.  The arrays the
 * kernels read are built from section 4 at the first call that needs them, and that call refuses, with a message starting
 * "zkey:", a value >= r, a section 4 without entries (pass the `.r1cs` then), and a domainSize below 2 or above 2^27.  The
 * doubled-Montgomery convention is checked here against this project's own writers (gwb_groth16_setup, gwb_groth16_setup_ptau)
 * and against the `.r1cs` path; no zkey written by snarkjs has been read by this code.
 *
 * Return and status conventions are those of graph_witness_r1cs.h (0 on success, 1 on failure with status filled).  The
 * curve points are uploaded to the device that is current at the first prove call and stay there; the device workspace
 * belongs to the zkey handle, grows on demand and is released by gwb_zkey_free.  A batch whose workspace would exceed
 * CWC_GROTH16_WORKSPACE_MB (read once per process, default 4096) runs in sub-batches.  Prove calls on one handle share
 * its workspace: enqueue them on one stream.  A handle may be used from one thread at a time.  A zkey that supplies the
 * witness map also owns that map's device state on the same device (coefficient arrays, twiddle and coset tables, the A / B
 * workspace of 2 n x 32 B per row, in sub-batches under CWC_R1CS_QAP_WORKSPACE_MB as for an `.r1cs` handle), released by
 * gwb_zkey_free too. */
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
 * >= r are reduced mod r) -> d_proofs [batch][256 B].  r: the circuit's `.r1cs` handle, or NULL for the witness map of the
 * zkey's section 4 (in all three prove calls).  rs: host array [batch][2][32 B] of canonical r, s (each below r), or
 * NULL: drawn uniformly from [0, r) by rejection sampling from getrandom().  Asynchronous on hip_stream with the ordering
 * contract of gwb_r1cs_check_batch_device; rs is read before the call returns. */
int gwb_groth16_prove_batch_device(gwb_zkey_t *z, gwb_r1cs_t *r, const void *d_witness, size_t n_witness, size_t batch,
                                   uint32_t form_in, const void *rs, void *d_proofs, void *hip_stream, gw_status_t *status);
/* The same with host rows (canonical) and host proofs; synchronous. */
int gwb_groth16_prove_batch_host(gwb_zkey_t *z, gwb_r1cs_t *r, const void *witness, size_t n_witness, size_t batch,
                                 const void *rs, void *proofs, gw_status_t *status);
/* One `.wtns` image, validated as gwb_r1cs_check_wtns validates it (BN254's r, section sizes, elements below r; nWitness
 * against the r1cs, or against the zkey's nVars when r is NULL) -> proof [256 B]; rs is [2][32 B] or NULL. */
int gwb_groth16_prove_wtns(gwb_zkey_t *z, gwb_r1cs_t *r, const void *wtns, size_t wtns_len, const void *rs, void *proof,
                           gw_status_t *status);
/* Measurement aid (as gwb_r1cs_qap_time_phases): with on != 0, later prove calls record HIP events around their phases (for
 * the last sub-batch of a call); gwb_groth16_phase_ms waits for the last call and writes ms[5] = witness map, scalar
 * preparation and sort, G1 MSMs (A, B1, C, H), G2 MSM (B2), assembly. */
int gwb_groth16_time_phases(gwb_zkey_t *z, int on);
int gwb_groth16_phase_ms(gwb_zkey_t *z, float *ms);

/* ---- The witness map of section 4 on its own: the counterparts of gwb_r1cs_qap_info, gwb_r1cs_qap_batch_device,
 * gwb_r1cs_qap_batch_host and gwb_r1cs_set_tile_width, with the same contracts (h in natural order, canonical or Montgomery;
 * n_witness == nVars).  n_rows of the info is 1 + the largest constraint index of any entry.  Each builds the map if it is
 * not built yet, so each can return the first-use refusals above. */
int gwb_zkey_qap_info(gwb_zkey_t *z, gwb_r1cs_qap_info_t *info, gw_status_t *status);
int gwb_zkey_qap_batch_device(gwb_zkey_t *z, const void *d_witness, size_t n_witness, size_t batch, uint32_t form_in, void *d_h,
                              uint32_t form_out, void *hip_stream, gw_status_t *status);
int gwb_zkey_qap_batch_host(gwb_zkey_t *z, const void *witness, size_t n_witness, size_t batch, void *h, uint32_t form_out,
                            gw_status_t *status);
int gwb_zkey_set_tile_width(gwb_zkey_t *z, uint32_t tile_width);
/* Does the zkey belong to this `.r1cs`?  Host only: no device is touched.  Section 4, summed per (matrix, constraint, signal)
 * with zero sums dropped, is compared with the A and B combinations of the `.r1cs` (summed and dropped likewise) plus the
 * nPublic + 1 public rows, then the size fields as the prove calls compare them.  Returns 0 when all agree.  Otherwise 1, and
 * the message names the smallest (constraint, matrix, signal) at which the two differ -- "zkey: section 4 differs from the
 * r1cs at constraint 12, matrix B, signal 7" -- or, where the terms agree, the size field that does not.  A zkey does not hold
 * the C matrix, so the C sides of the `.r1cs` are not compared: two circuits that differ only there pass. */
int gwb_zkey_check_r1cs(const gwb_zkey_t *z, const gwb_r1cs_t *r, gw_status_t *status);
/* Are the key's G2 points in the order-r subgroup?  (The twist has order r (2q - r), so a point on the curve can carry a
 * component of small order; a proof made with such a B2 point is refused by every verifier.)  Checks beta2, gamma2, delta2 and
 * the nVars points of section 7 on the current device (gwb_bn254_g2_check_batch_device's method 0; synchronous; the upload is
 * temporary and does not touch the prover's copies).  Returns 0, or 1 with the first offender in this order:
 * "zkey: beta2 is not in the order-r subgroup of G2" (likewise gamma2, delta2), then "zkey: section 7 (B2) point 12 is not in the
 * order-r subgroup of G2 (3 of 70 points are not)" with the smallest index. */
int gwb_zkey_check_g2(gwb_zkey_t *z, gw_status_t *status);
/* Host only: the `.wtns` image as gwb_groth16_prove_wtns validates it before it reaches the device, and nWitness == nVars
 * (for a caller that wants every input parsed before a device call other than the prove call, as groth16-prove --check-g2). */
int gwb_zkey_check_wtns(const gwb_zkey_t *z, const void *wtns, size_t wtns_len, gw_status_t *status);

#ifdef __cplusplus
}
#endif
#endif /* CWC_AMD_GRAPH_WITNESS_GROTH16_H */
