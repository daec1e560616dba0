/* KZG polynomial commitments on an MI355X over a powers-of-tau file (`.ptau`): the file that the ceremony of
 * graph_witness_groth16_ceremony.h makes and gwb_ptau_prepare_phase2 prepares, used as a structured reference string.  Commit
 * to a polynomial given by coefficients or by evaluations, open it at a point, open several at one point under one witness
 * (folded openings), check openings with the pairing of the Groth16 verifier.  This is the layer PLONK and fflonk stand on;
 * neither is part of it.
 *
 * TRUST.  The SRS is whatever the file holds.  Nothing here vouches for it: GWB_KZG_CHECK_POWERS (gwb_ptau_check_powers over
 * the covered prefix) and gwb_ptau_verify do, and the ceremony behind the file has to have had one honest participant.  A file
 * written from known logs (every test file is one) lets its author open any commitment to any value.
 *
 * Definitions.
 *   SRS          T_i = tauG1[i] (section 2, 2^(power+1) - 1 points), tauG2 = tauG2[1] (section 3), and Lag_m[k], the 2^m points
 *                of level m of section 12 at point offset 2^m - 1, as gwb_ptau_prepare_phase2 writes them.
 *   polynomial   p = (c_0 .. c_{N-1}), N coefficients.  Scalars are 32 bytes little-endian.  A coefficient or an evaluation at or
 *                above r is reduced mod r on load, as a witness row is.  In verification a y or z at or above r is refused, not
 *                reduced.
 *   commit       C = sum_i c_i T_i
 *   commit_evals C = sum_k e_k Lag_m[k] for e_k = p(w^k), w the root of order N = 2^m of the QAP domain (graph_witness_r1cs.h),
 *                natural order.  This is commit of the polynomial of length N with these evaluations.
 *   open at z    s_i = sum_{j >= i} c_j z^(j-i).  y = p(z) = s_0; the quotient (p(X) - y) / (X - z) has the coefficients
 *                q_i = s_{i+1}, i = 0 .. N - 2, and W = sum_i q_i T_i.  For N <= 1 the quotient is empty and W is the point at
 *                infinity; for N = 0, y = 0.
 *   check        (C, z, y, W) is VALID when e(C - y G1 + z W, G2) = e(W, tauG2).  This form of e(C - y G1, G2) = e(W, tauG2 - z G2)
 *                has no special case at z = tau.
 *   points       go in and out as 64 bytes: canonical little-endian affine x, y; zero bytes are the point at infinity
 *                (GWB_FORM_CANONICAL of graph_witness_batch.h, as the linear-combination aids use it).
 *
 * Statuses of a checked row, the first rule that fails, in this order:
 *   GWB_KZG_SCALAR    y or z is at or above r
 *   GWB_KZG_POINT     C or W has a coordinate at or above q, or is neither on the curve nor the point at infinity
 *   GWB_KZG_EQUATION  the pairing equation does not hold
 * Every row has its own equation and its own two pairings; the batch is not folded into one randomised equation.  The pairing
 * path does not take the point at infinity, so a row with L = C - y G1 + z W or W at infinity is decided by point comparison and
 * its pairings run on the generators: W = O and L = O is VALID (that is C = y G1), exactly one of them at infinity is EQUATION
 * (e(W, tauG2) is 1 only for W = O, since tauG2 is refused at infinity by gwb_kzg_new).  GT values are compared as bytes: the
 * final exponent is exact.
 *
 * Folded openings: several polynomials at one point, one witness.
 *   group        K >= 1 polynomials p_0 .. p_{K-1} of the same length N (the caller pads shorter ones with zeros), one point z and
 *                one challenge gamma.  The folded polynomial is f = sum_k gamma^k p_k, with gamma^0 = 1 also for gamma = 0.
 *   open_fold    y_k = p_k(z) for every k, and one W, the witness of f at z: W = sum_i q_i T_i with q the quotient of f as `open`
 *                defines it.  Coefficients, z and gamma at or above r are reduced, as open reduces.  N <= 1 gives W = O, N = 0
 *                gives y_k = 0.
 *   verify_fold  of (C_0 .. C_{K-1}, z, gamma, y_0 .. y_{K-1}, W): with C_f = sum_k gamma^k C_k and y_f = sum_k gamma^k y_k the
 *                group is VALID when e(C_f - y_f G1 + z W, G2) = e(W, tauG2).  Its status is the first rule that fails:
 *                GWB_KZG_SCALAR (z, gamma or any y_k at or above r: refused, not reduced), GWB_KZG_POINT (any C_k, or W, fails
 *                the point rule above), GWB_KZG_EQUATION.  L = C_f - y_f G1 + z W or W at infinity is decided as for a single row.
 *   K = 1        is open / check of that polynomial, for any gamma.
 * TRUST.  The folded check binds each y_k to its C_k only if gamma was fixed after the C_k, z and the y_k, by the caller's
 * transcript (a hash of them, in a non-interactive protocol).  The library derives nothing: gamma is an argument.  A prover who
 * knows gamma before choosing the y_k can pass the check with wrong values.
 * Every group keeps its own equation, its own two pairings and its own status.  Groups at different points are not combined under
 * one random factor (PLONK's u): that would save pairings, and a verify call here costs the same for one row as for thousands.
 *
 * The polynomial side (r1cs/kzg.hip) evaluates and divides a batch of K (polynomial, point) pairs in one launch per role and
 * level; the commitments and witnesses go through gwb_bn254_g1_lincomb_device, once per polynomial, over the SRS prefix that the
 * handle keeps on the device in canonical form.  Quotients of a batch live in a workspace bounded by CWC_GROTH16_WORKSPACE_MB
 * (the prover's knob); larger batches run in sub-batches.
 *
 * Return and status conventions are those of graph_witness_r1cs.h: 0, or 1 with status->error_msg (malloc'd).  The host calls
 * are synchronous and run on the current device; the _device calls are asynchronous on hip_stream and take device arrays. */
#ifndef CWC_AMD_GRAPH_WITNESS_KZG_H
#define CWC_AMD_GRAPH_WITNESS_KZG_H

#include <stddef.h>
#include <stdint.h>

#include "graph_witness_groth16_ptau.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gwb_kzg gwb_kzg_t;

enum { GWB_KZG_VALID = 0, GWB_KZG_SCALAR = 1, GWB_KZG_POINT = 2, GWB_KZG_EQUATION = 3 };

#define GWB_KZG_CHECK_POWERS 1u

typedef struct {
  uint64_t max_len;  /* polynomials of up to this many coefficients */
  uint32_t power;    /* of the file */
  uint32_t prepared; /* 1: the file has its Lagrange sections, commit_evals works */
} gwb_kzg_info_t;

/* The handle over a `.ptau` image; what it needs of the image is copied, so the caller's bytes are free after the call.  Refused with "kzg: ..." before
 * the device is touched: max_len = 0, max_len > 2^(power+1) - 1, unknown flags; a malformed file gets the loader's "ptau: ..."
 * message, and so does a wrong point among T_0 .. T_{max_len-1} and tauG2 (coordinates, curve; tauG2 at infinity is refused).
 * With GWB_KZG_CHECK_POWERS the powers check runs first (gwb_ptau_check_powers for the smallest domain whose prefixes cover
 * max_len, the whole-file sums when only they do) and its "ptau: ..." verdict is the refusal; without the flag the call does not
 * touch a device.  T_0 .. T_{max_len-1} and tauG2 go to the current device at the first call that runs there, and the later
 * calls have to be made on that device; the Lagrange points of level m follow at the first gwb_kzg_commit_evals_* for that m.
 * What a call refuses about its arguments (N > max_len, an unprepared file, 2^m > max_len) it refuses before any of that. */
int gwb_kzg_new(const void *ptau, size_t len, uint64_t max_len, uint32_t flags, gwb_kzg_t **out, gw_status_t *status);
int gwb_kzg_info(const gwb_kzg_t *h, gwb_kzg_info_t *info);
void gwb_kzg_free(gwb_kzg_t *h);

/* polys [K][N][32] -> points [K][64].  N > max_len is refused; K = 0 does nothing; N = 0 commits to infinity. */
int gwb_kzg_commit_batch(gwb_kzg_t *h, const void *polys, size_t K, size_t N, void *points, gw_status_t *status);
int gwb_kzg_commit_batch_device(gwb_kzg_t *h, const void *d_polys, size_t K, size_t N, void *d_points, void *hip_stream, gw_status_t *status);
/* evals [K][2^m][32] -> points [K][64].  A file without section 12 gets GWB_PTAU_LAGRANGE_FILE's refusal; 2^m > max_len is refused. */
int gwb_kzg_commit_evals_batch(gwb_kzg_t *h, const void *evals, size_t K, uint32_t m, void *points, gw_status_t *status);
int gwb_kzg_commit_evals_batch_device(gwb_kzg_t *h, const void *d_evals, size_t K, uint32_t m, void *d_points, void *hip_stream,
                                      gw_status_t *status);
/* polys [K][N][32], zs [K][32] (reduced mod r) -> ys [K][32].  Reads no SRS point, so N is bounded by 2^31 - 1 only. */
int gwb_kzg_eval_batch(gwb_kzg_t *h, const void *polys, const void *zs, size_t K, size_t N, void *ys, gw_status_t *status);
int gwb_kzg_eval_batch_device(gwb_kzg_t *h, const void *d_polys, const void *d_zs, size_t K, size_t N, void *d_ys, void *hip_stream,
                              gw_status_t *status);
/* -> ys [K][32], proofs [K][64] (the points W).  N > max_len is refused. */
int gwb_kzg_open_batch(gwb_kzg_t *h, const void *polys, const void *zs, size_t K, size_t N, void *ys, void *proofs, gw_status_t *status);
int gwb_kzg_open_batch_device(gwb_kzg_t *h, const void *d_polys, const void *d_zs, size_t K, size_t N, void *d_ys, void *d_proofs,
                              void *hip_stream, gw_status_t *status);
/* commitments [K][64], zs [K][32], ys [K][32], proofs [K][64] -> status_out [K] uint32 (GWB_KZG_*) */
int gwb_kzg_verify_batch(gwb_kzg_t *h, const void *commitments, const void *zs, const void *ys, const void *proofs, size_t K,
                         void *status_out, gw_status_t *status);
int gwb_kzg_verify_batch_device(gwb_kzg_t *h, const void *d_commitments, const void *d_zs, const void *d_ys, const void *d_proofs, size_t K,
                                void *d_status, void *hip_stream, gw_status_t *status);

/* ms[4] of the handle's last open or verify call (HIP events, summed over its sub-batches): quotient, lincomb, prepare, pairing.
 * An open has no prepare and no pairing, a verify no quotient and no lincomb: those are 0.  A _device call is waited for.
 * 1 when no such call has completed yet. */
int gwb_kzg_phase_ms(gwb_kzg_t *h, float *ms);

/* Folded openings of G groups of K polynomials: polys [G][K][N][32], zs [G][32], gammas [G][32] -> ys [G][K][32], proofs [G][64].
 * One fold, one quotient and one linear combination per group whatever K is; the y_k are K evaluations.  Refused before the
 * device is touched: K = 0, N > max_len, G K > 2^31 - 1.  G = 0 does nothing.  The folded polynomials and their quotients live in
 * the workspace that CWC_GROTH16_WORKSPACE_MB bounds; more groups run in sub-batches. */
int gwb_kzg_open_fold_batch(gwb_kzg_t *h, const void *polys, const void *zs, const void *gammas, size_t G, size_t K, size_t N, void *ys,
                            void *proofs, gw_status_t *status);
int gwb_kzg_open_fold_batch_device(gwb_kzg_t *h, const void *d_polys, const void *d_zs, const void *d_gammas, size_t G, size_t K, size_t N,
                                   void *d_ys, void *d_proofs, void *hip_stream, gw_status_t *status);
/* commitments [G][K][64], zs [G][32], gammas [G][32], ys [G][K][32], proofs [G][64] -> status_out [G] uint32 (GWB_KZG_*).  The K + 2
 * multiplications of a group run side by side, 64 to a workgroup, and are added in a tree.  K = 0 and G K > 2^31 - 1 are refused. */
int gwb_kzg_verify_fold_batch(gwb_kzg_t *h, const void *commitments, const void *zs, const void *gammas, const void *ys, const void *proofs,
                              size_t G, size_t K, void *status_out, gw_status_t *status);
int gwb_kzg_verify_fold_batch_device(gwb_kzg_t *h, const void *d_commitments, const void *d_zs, const void *d_gammas, const void *d_ys,
                                     const void *d_proofs, size_t G, size_t K, void *d_status, void *hip_stream, gw_status_t *status);
/* ms[6] of the handle's last open_fold or verify_fold call, as gwb_kzg_phase_ms: fold, evals (the y_k), quotient, lincomb, prepare
 * (the point fold and the pairing inputs), pairing.  An open_fold has no prepare and no pairing, a verify_fold only those.  The
 * folded calls leave gwb_kzg_phase_ms's values alone, and the other calls these. */
int gwb_kzg_fold_phase_ms(gwb_kzg_t *h, float *ms);

/* Test and measurement aids of the folded openings' kernels, handle-free.
 * gwb_kzg_fold_device: d_polys [G][K][N][32], d_gammas [G][32], any values -> d_out [G][N][32] = sum_k gamma^k p_k, canonical.
 * Asynchronous on hip_stream.
 * gwb_kzg_fold_points_device: d_points [G][K][64], d_gammas [G][32] (reduced) -> d_out [G][64] = sum_k gamma^k C_k.  A point that
 * fails the point rule makes the call fail with the first such group in the message; to say so the call waits for hip_stream. */
int gwb_kzg_fold_device(const void *d_polys, const void *d_gammas, size_t G, size_t K, size_t N, void *d_out, void *hip_stream,
                        gw_status_t *status);
int gwb_kzg_fold_points_device(const void *d_points, const void *d_gammas, size_t G, size_t K, void *d_out, void *hip_stream,
                               gw_status_t *status);

/* Test and measurement aid of the evaluate-and-quotient kernels, handle-free: d_polys [K][N][32], d_zs [K][32] -> d_ys [K][32]
 * and d_qs [K][N-1][32], canonical, with workgroups that own `tile` consecutive coefficients (one of gwb_kzg_tiles; 0 = the
 * production tile).  A polynomial longer than a tile takes one more level of the recursion per factor `tile`.  Asynchronous on
 * hip_stream (the workspace is allocated and freed in stream order). */
int gwb_kzg_eval_quotient_device(const void *d_polys, const void *d_zs, size_t K, size_t N, uint32_t tile, void *d_ys, void *d_qs,
                                 void *hip_stream, gw_status_t *status);
/* The tile sizes instantiated, smallest first: *n in = room in tiles, out = their number. */
int gwb_kzg_tiles(uint32_t *tiles, size_t *n);

#ifdef __cplusplus
}
#endif
#endif /* CWC_AMD_GRAPH_WITNESS_KZG_H */
