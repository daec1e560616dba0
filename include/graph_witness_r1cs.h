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

#ifdef __cplusplus
}
#endif
#endif /* CWC_AMD_GRAPH_WITNESS_R1CS_H */
