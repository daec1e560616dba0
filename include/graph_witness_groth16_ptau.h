/* Groth16 proving keys on an MI355X from a circuit's `.r1cs` and a powers-of-tau ceremony file (`.ptau`): what
 * `snarkjs groth16 setup circuit.r1cs pot.ptau circuit.zkey` does, with tau, alpha and beta taken from the ceremony instead of
 * from the caller (graph_witness_groth16_setup.h is the setup from a known trapdoor).
 *
 * TRUST.  tau, alpha and beta are those of the ceremony behind the file: nobody knows them if one participant of that
 * ceremony was honest, and this library does not verify records made by snarkjs (gwb_ptau_verify of
 * graph_witness_groth16_ceremony.h checks its own, and the whole file);
 * gwb_ptau_check_powers checks, when asked, that the points a setup reads are powers of one tau at all.
 * gamma is 1, as in snarkjs.  delta is the caller's:
 *   delta = 1 gives the state of snarkjs `zkey new`: a key that is to be handed to a phase-2 ceremony, NOT to be used, since
 *   everybody knows its delta and knowing delta alone is enough to forge proofs;
 *   delta = NULL draws delta, applies it and zeroes it on the host and on the device before the call returns.  The key's
 *   soundness then rests on two things: the ceremony behind the ptau, and the runner of this call discarding delta.  This is
 *   a single-party phase 2, not an MPC phase 2: the file's section 10 records no contribution.
 *   A supplied delta other than 1 makes a reproducible key whose delta the supplier knows (tests).
 *
 * Definition.  n = 2^p is the circuit's QAP domain (gwb_r1cs_qap_info), w_N the generator of the domain of N = 2^m points
 * (graph_witness_r1cs.h: w_n, and g = w_2n).  From the file's monomial sections take the prefixes T1_i = tau^i G1 (i < 2n),
 * T2_i = tau^i G2, AT_i = alpha tau^i G1, BT_i = beta tau^i G1 (i < n).  For a point sequence P of length N = 2^m
 *   Lag_m(P)_k = (1 / N) sum_i w_N^(-k i) P_i           (the inverse DFT over the group: tau^i G -> L_k(tau) G)
 * and L1 = Lag_p(T1), L2 = Lag_p(T2), LA = Lag_p(AT), LB = Lag_p(BT), M = Lag_(p+1)(T1).  With the R1CS's nC constraints
 * (A_k, B_k, C_k), nW wires and nPub public signals:
 *   section 5 (A):   A_i  = sum_k A_k[i] L1_k  (+ L1_{nC+i} for i <= nPub)
 *   section 6 (B1):  B1_i = sum_k B_k[i] L1_k             section 7 (B2):  B2_i = sum_k B_k[i] L2_k
 *   K_i = sum_k A_k[i] LB_k (+ LB_{nC+i} for i <= nPub) + sum_k B_k[i] LA_k + sum_k C_k[i] L1_k
 *   section 3 (IC):  IC_i = K_i for i <= nPub             section 8 (C):   C_{i-nPub-1} = (1 / delta) K_i for i > nPub
 *   section 9 (H):   H_j  = (1 / delta) M_{2j+1}
 *   header:          alpha1 = AT_0, beta1 = BT_0, beta2 = the file's section 6, gamma2 = G2, delta1 = delta G1, delta2 = delta G2
 * Sections 4 and 10 and the section order are those of gwb_groth16_setup.  For a file whose logs are (tau, alpha, beta) the
 * key is, byte for byte, gwb_groth16_setup's with the trapdoor (tau, alpha, beta, 1, delta).
 *
 * The `.ptau` file (iden3 binfile "ptau" v1; r1cs/ptau.cc has the layout).  The loader takes any bytes, an mmap'd file
 * included, and reads only the header, the section table and the prefixes named above.  It refuses with a message: a wrong
 * magic or version; n8 != 32 or a q that is not BN254's; power > 28; a missing, duplicate or mis-sized section 1 to 6; a
 * coordinate >= q or a point off its curve among those it reads (naming section and index); T1_0 != G1 or T2_0 != G2; and a
 * circuit with p + 1 > power.  snarkjs also accepts p = power, through a truncated top level of M; that case is left out
 * here.  Like the zkey loader it does not check G2 points for subgroup membership; gwb_ptau_check_g2 does, on the device,
 * when asked.  The layout is restated from snarkjs's
 * writer and has not been cross-checked against snarkjs itself (no snarkjs output is available to this project).
 *
 * Lagrange source.  A file that went through `powersoftau prepare phase2` carries L1, L2, LA, LB and M already (sections 12
 * to 15).  GWB_PTAU_LAGRANGE_AUTO reads them when they are present and computes them otherwise, _FILE fails with a message
 * when they are absent, _COMPUTE ignores them.  gwb_ptau_prepare_phase2 writes them; a setup does not compare what they hold
 * with the monomial sections, gwb_ptau_check_lagrange does.
 *
 * Return and status conventions are those of graph_witness_r1cs.h.  gwb_groth16_setup_ptau is synchronous and runs on the
 * current device. */
#ifndef CWC_AMD_GRAPH_WITNESS_GROTH16_PTAU_H
#define CWC_AMD_GRAPH_WITNESS_GROTH16_PTAU_H

#include <stddef.h>
#include <stdint.h>

#include "graph_witness_groth16_setup.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { GWB_PTAU_LAGRANGE_AUTO = 0, GWB_PTAU_LAGRANGE_FILE = 1, GWB_PTAU_LAGRANGE_COMPUTE = 2 };

typedef struct {
  uint32_t power;           /* the file holds tau^i G1 for i < 2^(power+1) - 1 */
  uint32_t ceremony_power;  /* the power of the ceremony the file was cut from */
  uint32_t prepared;        /* 1: sections 12 to 15 are present with their expected sizes */
  uint32_t n_contributions; /* as section 7 states it; the records are not read */
} gwb_ptau_info_t;

/* Host only, no device: header and section table, the generators at T1_0 and T2_0. */
int gwb_ptau_info(const void *data, size_t len, gwb_ptau_info_t *info, gw_status_t *status);

/* Host only, no device: everything gwb_groth16_setup_ptau would refuse about the file for a circuit of domain
 * 2^domain_power under lagrange_mode, with the same messages; the points are checked on the host (the setup checks them on
 * the device). */
int gwb_ptau_check(const void *data, size_t len, uint32_t domain_power, uint32_t lagrange_mode, gw_status_t *status);

/* G2 subgroup membership of the G2 points a setup for the domain 2^domain_power reads under lagrange_mode: beta2 (section 6)
 * and tauG2[0 .. n) (section 3) when the Lagrange forms are computed, or tauG2[0] and the n points of level domain_power of
 * section 13 when they come from the file.  First everything gwb_ptau_check refuses about the header, the section table, the
 * plan and alpha1, beta1, beta2, on the host and with its messages; then the points go to the current device in bounded pieces
 * (gwb_bn254_g2_check_batch_device's method 0; synchronous).  Returns 0, or 1 with the first offender, section 6 before 3 before
 * 13: "ptau: section 3 (tauG2) point 5 is not in the order-r subgroup of G2" (a coordinate >= q or a point off the curve among
 * them is named as gwb_ptau_check names it). */
int gwb_ptau_check_g2(const void *data, size_t len, uint32_t domain_power, uint32_t lagrange_mode, gw_status_t *status);

/* Checks that the monomial prefixes a setup for the domain n = 2^domain_power reads under GWB_PTAU_LAGRANGE_COMPUTE are what their
 * sections' names say: T1 = tauG1[0 .. 2n), T2 = tauG2[0 .. n), AT = alphaTauG1[0 .. n), BT = betaTauG1[0 .. n) and beta2.  First
 * everything gwb_ptau_check refuses, with its messages (returns 2); then the subgroup rule of gwb_ptau_check_g2 (the pairing is
 * bilinear on the order-r subgroup only; returns 1 with its message); then, with 128-bit rho_0 .. rho_{2n-2} cut from `seed` as
 * gwb_zkey_verify_step cuts them (32 bytes, or NULL to draw them), six sums computed on the device from points that go there in
 * pieces of CWC_CONTRIBUTE_CHUNK:
 *   U = sum_{i<2n-1} rho_i T1_{i+1}   V = sum_{i<2n-1} rho_i T1_i   V_n = sum_{i<n} rho_i T1_i
 *   S_A = sum_{i<n} rho_i AT_i        S_B = sum_{i<n} rho_i BT_i    S_2 = sum_{i<n} rho_i T2_i (in G2)
 * and five equations in one batched pairing launch; the first that fails is the verdict (returns 1):
 *   e(U, G2) = e(V, T2_1)        "ptau: section 2 (tauG1): the first 2n points are not consecutive powers of the tau of section 3"
 *   e(G1, S_2) = e(V_n, G2)      "ptau: section 3 (tauG2): ..."
 *   e(S_A, G2) = e(AT_0, S_2)    "ptau: section 4 (alphaTauG1): ..."
 *   e(S_B, G2) = e(BT_0, S_2)    "ptau: section 5 (betaTauG1): ..."
 *   e(BT_0, G2) = e(G1, beta2)   "ptau: section 6 (betaG2): ..."
 * A side with a point at infinity is 1: one such side alone fails its equation, two pass.  A file with a wrong point among the
 * prefixes passes with probability about 2^-128 over the seed.  NOT checked: the points beyond the prefixes (tauG1[2n] may be
 * anything; gwb_ptau_verify of graph_witness_groth16_ceremony.h checks the whole file); the Lagrange sections 12 to 15; records
 * made by snarkjs in section 7, whose challenge derivation cannot be restated here.  Returns 2 for anything that is not a verdict.  Synchronous, on the current device. */
int gwb_ptau_check_powers(const void *data, size_t len, uint32_t domain_power, const uint8_t *seed, gw_status_t *status);

/* What `powersoftau prepare phase2` does: the file with its Lagrange sections 12 to 15 made on the current device from its
 * monomial sections 2 to 5.  Section 12 + j (j = 0 .. 3) holds the levels m = 0 .. power of section 2 + j one after the other,
 * level m being the 2^m points Lag_m(P_0 .. P_{2^m - 1}) of the section's first 2^m points P, at point offset 2^m - 1.  Section 12
 * has one level more, m = power + 1: section 2 holds only 2^(power+1) - 1 points, the missing last input is the point at
 * infinity, and the level is Lag_(power+1)(T1_0, .., T1_{2n-2}, O) for n = 2^power, as in snarkjs (a setup never reads it: it
 * needs p + 1 <= power).  So the sections hold 4n - 1 G1, 2n - 1 G2, 2n - 1 G1 and 2n - 1 G1 points.
 * *out is a complete `.ptau` image, released with gwb_groth16_setup_free: every section of the input other than 12 to 15 byte
 * for byte and in the input's order, ids this library does not know included, then sections 12, 13, 14 and 15; an input that
 * already has them gets them replaced.  The file is parsed as gwb_ptau_info parses it, and the size rules below are applied,
 * before the device is touched; every monomial point is then checked on the device as the setup checks the ones it reads
 * (coordinates, curve; the same messages).  One section at a time has all its levels on the device in extended coordinates
 * ((4n - 1) 128 bytes for section 12, (2n - 1) 256 for section 13): a file for which that, with the uploaded prefix, the twiddles
 * and one piece of output, is more than CWC_GROTH16_WORKSPACE_MB (the prover's knob, read once per process; 4096 without it) is
 * refused with a message naming the power and the bytes, and so is a power above 27.  The results come
 * back in pieces of CWC_CONTRIBUTE_CHUNK points.  No snarkjs-prepared file was available to compare the container or the
 * points with.  Returns 0 or 1.  Synchronous. */
int gwb_ptau_prepare_phase2(const void *ptau, size_t ptau_len, void **out, size_t *out_len, gw_status_t *status);

/* ms[4] of the last gwb_ptau_prepare_phase2 call of the process (HIP events, summed over the four sections): load (upload,
 * point checks and the per-level bit reversal), idft_g1, idft_g2 (the stages and the factors 1 / 2^m), affine (conversion and
 * the copies back).  1 when no call has completed yet. */
int gwb_ptau_prepare_phase_ms(float *ms);

#define GWB_PTAU_ALL_LEVELS 0xffffffffu

/* Checks the Lagrange sections 12 to 15 of a prepared file against its monomial sections 2 to 5 on the current device.  With
 * domain_power = p the levels a setup for the domain 2^p reads under GWB_PTAU_LAGRANGE_FILE: level p of sections 12 to 15 and
 * level p + 1 of section 12; with GWB_PTAU_ALL_LEVELS every level of every section (section 12's last level as
 * gwb_ptau_prepare_phase2 defines it).  First, returning 2 with their own messages: everything gwb_ptau_check refuses about the
 * header, the section table and the plan (a file without sections 12 to 15 gets GWB_PTAU_LAGRANGE_FILE's refusal), then a
 * coordinate >= q or a point off its curve among the points read, Lagrange and monomial.  Then, for section 13, the subgroup
 * rule of gwb_ptau_check_g2 over the Lagrange points read (returns 1): the equation below sees a component of small order
 * with probability 1 / order only.  Then per section, with 128-bit rho_{m,k} cut from `seed` (32 bytes, or NULL to draw them
 * after the file is seen) as gwb_zkey_verify_step cuts them, rho_{m,k} = rho of index 2^m - 1 + k:
 *   sum_m sum_k rho_{m,k} Lag_m[k]  =  sum_i c_i P_i,   c_i = sum_{m: i < 2^m} (1 / 2^m) sum_k w_(2^m)^(-k i) rho_{m,k}
 * over the checked levels m; the transform's matrix is symmetric, so c is the sum of Lag_m of the rho of level m, and it is
 * computed on the device.  Both sides are sums the device forms (the left with the 128-bit rho, the right with the full-width
 * c) and they are compared as points: no pairing.  For the last level of section 12, c_{2n-1} multiplies O and is dropped.  In
 * domain mode every level has an equation of its own and the verdict names it: "ptau: section 14 (lagrange alphaTauG1) level 3
 * does not hold the Lagrange forms of section 4"; for all levels a section has one equation and one full-width combination
 * of its monomial points, and after a failure the levels are tried one by one to name the first: "ptau: section 12 (lagrange
 * tauG1) does not hold the Lagrange forms of section 2: level 4 is the first that does not".  Sections are checked in the order
 * 12 to 15.  A file with a wrong point among the checked levels passes with probability about 2^-128 over the seed.  NOT
 * checked: that sections 2 to 5 are powers of one tau (gwb_ptau_check_powers).  Returns 2 for anything that is not a verdict.
 * Synchronous. */
int gwb_ptau_check_lagrange(const void *data, size_t len, uint32_t domain_power, const uint8_t *seed, gw_status_t *status);

/* Measurement and test aids of the Lagrange check's right-hand side: d_points [n][64 B] (g1) or [128 B] (g2) affine in `form`
 * (GWB_FORM_CANONICAL or GWB_FORM_MONTGOMERY of graph_witness_batch.h; zero bytes = infinity, not checked) and d_scalars [n][32 B]
 * canonical little-endian values below r -> d_out, one point in the same form: sum_i scalar_i P_i.  Beside
 * gwb_bn254_g1_lincomb128_device and its G2 twin (graph_witness_groth16_contribute.h), whose kernels these instantiate with
 * eight scalar words.  Asynchronous on hip_stream. */
int gwb_bn254_g1_lincomb_device(const void *d_points, const void *d_scalars, size_t n, uint32_t form, void *d_out, void *hip_stream,
                                gw_status_t *status);
int gwb_bn254_g2_lincomb_device(const void *d_points, const void *d_scalars, size_t n, uint32_t form, void *d_out, void *hip_stream,
                                gw_status_t *status);

/* delta: 32 bytes canonical little-endian in [1, r), or NULL to draw it (the prover's rejection sampler over getrandom()).
 * *zkey is released with gwb_groth16_setup_free. */
int gwb_groth16_setup_ptau(gwb_r1cs_t *r, const void *ptau, size_t ptau_len, const uint8_t *delta, uint32_t lagrange_mode,
                           void **zkey, size_t *zkey_len, gw_status_t *status);

/* Measurement and test aid, like gwb_bn254_gen_mul_batch_device: d_points [2^log_n][64 B] (group 1) or [128 B] (group 2),
 * canonical little-endian affine coordinates, zero bytes = infinity (the points are not checked) -> d_out, the same form:
 * Lag_(log_n) of the sequence, in natural order.  1 <= log_n <= 27.  Asynchronous on hip_stream. */
int gwb_bn254_point_idft_batch_device(const void *d_points, uint32_t log_n, uint32_t group, void *d_out, void *hip_stream,
                                      gw_status_t *status);

/* ms[7] of the last gwb_groth16_setup_ptau call of the process (HIP events): point_check (loading and checking the points
 * read), idft_g1, idft_g2 (0 when the Lagrange forms came from the file), column_sums_g1, column_sums_g2, delta_scale,
 * affine.  1 when no call has completed yet. */
int gwb_groth16_setup_ptau_phase_ms(float *ms);

#ifdef __cplusplus
}
#endif
#endif /* CWC_AMD_GRAPH_WITNESS_GROTH16_PTAU_H */
