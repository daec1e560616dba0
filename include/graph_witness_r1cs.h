/* R1CS satisfaction check of witness batches on an MI355X.
 *
 * The graph the witness calculator evaluates keeps only a circuit's assignments (`<--` / `<==`); the `===` constraints are
 * dropped when the graph is built, so a wrong input (a zero divisor, a value out of range, a bad signature) still yields a
 * witness, and the status words of graph_witness_batch.h do not flag it.  These functions load the circuit's `.r1cs` file
 * (the iden3 binfile "r1cs" v1 format circom writes) and check every constraint
 *
 *     (sum_A a * w[wire]) * (sum_B b * w[wire]) - sum_C c * w[wire] == 0  (mod r)
 *
 * for every witness row of a batch, on the device, reporting per row the smallest failing constraint index and the number
 * of failing constraints.  Wire i is element i of a witness row (the `.wtns` section-2 order); wire 0 is the constant 1.
 * BN254 only; files with custom gates (sections 4 and 5, `circom --O2 ... custom_templates`) are rejected.
 *
 * Return and status conventions are those of graph_witness_batch.h: 0 on success, 1 on failure with status filled (status
 * may be NULL).  A handle may be used from one thread at a time.  Its constraint arrays are uploaded to the device that is
 * current at the first check call and stay there for the life of the handle; later checks must run on that device.
 * Built as libcwc_r1cs.so, independent of libcircom_witnesscalc_amd.so.
 */
#ifndef CWC_AMD_GRAPH_WITNESS_R1CS_H
#define CWC_AMD_GRAPH_WITNESS_R1CS_H

#include <stddef.h>
#include <stdint.h>

#include "graph_witness_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gwb_r1cs gwb_r1cs_t;

typedef struct {
  uint32_t n_wires, n_pub_out, n_pub_in, n_prv_in, n_constraints;
  uint64_t n_labels;
  uint64_t n_factors_a, n_factors_b, n_factors_c; /* (wire, coefficient) pairs over all constraints, per combination */
} gwb_r1cs_info_t;

/* "No failing constraint" in first_failed. */
#define GWB_R1CS_SATISFIED 0xffffffffu

/* Parse + validate a `.r1cs` image (hostile bytes are refused with a message, never read out of bounds). */
int gwb_r1cs_load(const void *data, size_t len, gwb_r1cs_t **out, gw_status_t *status);
void gwb_r1cs_free(gwb_r1cs_t *r);
int gwb_r1cs_info(const gwb_r1cs_t *r, gwb_r1cs_info_t *info);

/* Witness rows per wavefront of the check kernel: a power of two in 1..64, or 0 = choose from the batch size (default). */
int gwb_r1cs_set_tile_width(gwb_r1cs_t *r, uint32_t tile_width);

/* Device rows [batch][n_witness][32 B] little-endian, in form GWB_FORM_CANONICAL or GWB_FORM_MONTGOMERY (the rows of
 * gwb_calc_witness_batch_device / _handoff); n_witness must equal the file's nWires.  Writes d_first_failed[s] (smallest
 * failing original constraint index, or GWB_R1CS_SATISFIED) and d_n_failed[s] ([batch] u32 device arrays).  Asynchronous
 * on hip_stream (hipStream_t or NULL): enqueue it behind gwb_calc_witness_batch_handoff on the same stream, or wait for
 * the hand-off event first. */
int gwb_r1cs_check_batch_device(gwb_r1cs_t *r, const void *d_witness, size_t n_witness, size_t batch, uint32_t form,
                                uint32_t *d_first_failed, uint32_t *d_n_failed, void *hip_stream, gw_status_t *status);
/* The same with host rows (canonical form) and host outputs; synchronous. */
int gwb_r1cs_check_batch_host(gwb_r1cs_t *r, const void *witness, size_t n_witness, size_t batch,
                              uint32_t *first_failed, uint32_t *n_failed, gw_status_t *status);
/* One `.wtns` image (what snarkjs `wtns check` does): *first_failed = GWB_R1CS_SATISFIED when every constraint holds.
 * An image whose prime is not BN254's r, whose length disagrees with its sections or whose elements are not below r is
 * refused (return 1). */
int gwb_r1cs_check_wtns(gwb_r1cs_t *r, const void *wtns, size_t wtns_len, uint32_t *first_failed, uint32_t *n_failed,
                        gw_status_t *status);

/* ---- Groth16 witness map: the quotient evaluations h of witness rows (what snarkjs `groth16 prove` and rapidsnark feed
 * to the MSM against the zkey's H points).
 *
 * For a loaded `.r1cs` with nC constraints, nPub = nPubOut + nPubIn, and a witness row w (wire i = element i, wire 0 = 1):
 *   Rows.    N = nC + nPub + 1.  Row i < nC is constraint i in file order: a_i = sum_A coeff * w[wire],
 *            b_i = sum_B coeff * w[wire] (the file's C side is not read).  Row nC + s, s = 0..nPub, is a = w[s], b = 0
 *            (the input constraints snarkjs `zkey new` adds for the constant wire and every public signal).  Rows N..n-1
 *            are a = b = 0.  c_i = a_i * b_i for every row (snarkjs buildABC1, rapidsnark), so a witness that does not
 *            satisfy the system still gets its h.
 *   Domain.  n = 2^p, p the smallest integer >= 1 with 2^p >= N; p > 27 is refused (the coset needs a 2n-th root of unity
 *            and the 2-adicity of r is 28).
 *   Roots.   w_28 = 5^((r-1)/2^28) mod r (5 is the smallest quadratic non-residue; ffjavascript's and arkworks' root),
 *            w_n = w_28^(2^(28-p)), g = w_2n = w_28^(2^(27-p)).
 *   Output.  A(X) is the polynomial of degree < n with A(w_n^i) = a_i, B and C likewise;
 *            h_j = A(g w_n^j) * B(g w_n^j) - C(g w_n^j) for j = 0..n-1, natural order (snarkjs's buffPodd_T),
 *            canonical (GWB_FORM_CANONICAL) or Montgomery (GWB_FORM_MONTGOMERY) as asked.
 *   Input.   Rows canonical or Montgomery, as for the check; elements >= r in a row are reduced mod r.
 *
 * The twiddle and coset tables (2 n x 32 B) are built on the handle's device at the first QAP call and kept.  The device
 * workspace (the A and B evaluations, workspace_bytes_per_row per row) belongs to the handle, grows on demand and is
 * released by gwb_r1cs_free.  A batch larger than the workspace cap (environment variable CWC_R1CS_QAP_WORKSPACE_MB,
 * read once per process, default 4096) runs in sub-batches of cap / workspace_bytes_per_row rows (at least one).
 * QAP calls on one handle share its workspace: enqueue them on one stream, or wait for the previous call before the next. */
typedef struct {
  uint64_t n_rows;                  /* N = nC + nPub + 1 */
  uint32_t domain_power;            /* p */
  uint64_t domain_size;             /* n = 2^p */
  uint64_t workspace_bytes_per_row; /* device workspace per witness row */
} gwb_r1cs_qap_info_t;

/* Fails (return 1, status filled) for p > 27. */
int gwb_r1cs_qap_info(const gwb_r1cs_t *r, gwb_r1cs_qap_info_t *info, gw_status_t *status);
/* Device rows [batch][n_witness][32 B] in form_in (n_witness must equal nWires) -> d_h [batch][n][32 B] in form_out.
 * Asynchronous on hip_stream, with the ordering contract of gwb_r1cs_check_batch_device. */
int gwb_r1cs_qap_batch_device(gwb_r1cs_t *r, const void *d_witness, size_t n_witness, size_t batch, uint32_t form_in, void *d_h,
                              uint32_t form_out, void *hip_stream, gw_status_t *status);
/* The same with host rows (canonical) and host h [batch][n][32 B]; synchronous. */
int gwb_r1cs_qap_batch_host(gwb_r1cs_t *r, const void *witness, size_t n_witness, size_t batch, void *h, uint32_t form_out,
                            gw_status_t *status);
/* One `.wtns` image, validated as gwb_r1cs_check_wtns validates it -> h_out [n][32 B] in form_out. */
int gwb_r1cs_qap_wtns(gwb_r1cs_t *r, const void *wtns, size_t wtns_len, void *h_out, uint32_t form_out, gw_status_t *status);
/* Measurement aid: with on != 0, later QAP calls record HIP events around their phases (for the last sub-batch of a call);
 * gwb_r1cs_qap_phase_ms waits for the last call and writes ms[4] = evaluation (a, b, c and padding), inverse outer passes,
 * the fused inner pass (inverse, coset scaling, forward), forward outer passes with A B - C.  Return 0 on success. */
int gwb_r1cs_qap_time_phases(gwb_r1cs_t *r, int on);
int gwb_r1cs_qap_phase_ms(gwb_r1cs_t *r, float *ms);
/* Measurement aid: the current device's rate of dependent BN254 Montgomery products (the fr_mul the kernels use), from a
 * short probe kernel (8 waves per SIMD, 4 independent chains per lane). */
int gwb_r1cs_modmul_rate(double *products_per_s);

#ifdef __cplusplus
}
#endif
#endif /* CWC_AMD_GRAPH_WITNESS_R1CS_H */
