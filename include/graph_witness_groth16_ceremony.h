/* A powers-of-tau ceremony on an MI355X: what snarkjs `powersoftau new` and `powersoftau contribute` do to a `.ptau`, with this
 * library's own transcript (below: the records are NOT interchangeable with snarkjs's).  The file's layout is in r1cs/ptau.cc,
 * what is made from such a file in graph_witness_groth16_ptau.h.
 *
 * A new file of power P holds tau = alpha = beta = 1: every point is its group's generator.  A contribution with the secrets
 * tau', alpha', beta' multiplies every point by its own scalar:
 *   tauG1[i] <- tau'^i tauG1[i] (i < 2^(P+1) - 1)      tauG2[i] <- tau'^i tauG2[i] (i < 2^P)
 *   alphaTauG1[i] <- alpha' tau'^i alphaTauG1[i]       betaTauG1[i] <- beta' tau'^i betaTauG1[i] (i < 2^P)      betaG2 <- beta' betaG2
 * So a file written from the logs (tau, alpha, beta) holds after the contribution exactly the bytes of the file written from
 * (tau tau', alpha alpha', beta beta').  Section 1 and every section id this library does not know are carried byte for byte
 * in the input's order; section 7 gets one record more; sections 12 to 15 (`powersoftau prepare phase2`) are DROPPED: they
 * would be the Lagrange forms of the old tau (gwb_ptau_prepare_phase2 makes them again).
 *
 * Trust.  After contributions by several parties tau, alpha and beta are known to nobody unless ALL of them kept and pooled
 * their secrets; one honest participant who discarded them is enough.  Each call draws its secrets (unless given) and zeroes
 * them, the three nonces, the table of tau'^(2^b) and every piece's scalars on the host and on the device before it returns,
 * on error paths too.  Secrets passed in by the caller are the caller's to discard.
 *
 * Section 7 (the field order is snarkjs's writeContribution as far as it is remembered; no snarkjs source or output was
 * available to check it; points affine, Montgomery, little-endian as everywhere in the file):
 *   u32 nContributions | per record:
 *     the after-values  tauG1 = tauG1[1] 64 B | tauG2 = tauG2[1] 128 B | alphaG1 = alphaTauG1[0] 64 B | betaG1 = betaTauG1[0] 64 B |
 *                       betaG2 128 B
 *     the key           tau_g1_s | tau_g1_sx | alpha_g1_s | alpha_g1_sx | beta_g1_s | beta_g1_sx (G1, 64 B each) |
 *                       tau_g2_spx | alpha_g2_spx | beta_g2_spx (G2, 128 B each)
 *     216 B partialHash (snarkjs's saved hash state: written as zeros here, ignored when read, kept byte for byte in records
 *                       that are carried)
 *     64 B nextChallenge
 *     u32 type (0 = contribution, 1 = beacon) | u32 paramsLen | params
 *   params: the tagged items of the zkey's section 10:  01 len name[len]  |  02 numIterationsExp  |  03 len beaconHash[len]
 * Records of type 1 are made by gwb_ptau_beacon and checked against their parameters by the verifications below
 * (graph_witness_groth16_beacon.h); a contribution carries them byte for byte.  The reader refuses, with a message that starts
 * "ptau: section 7": a truncated section, a record count the section cannot hold, a paramsLen or an item length that runs past
 * its end, an unknown tag or type, a coordinate >= q, a point off its curve, trailing bytes.  A file without section 7 has no
 * records.
 *
 * Transcript.  H is unkeyed BLAKE2b-512; U1, U2 and hash_to_g2 are those of graph_witness_groth16_contribute.h, unchanged.
 *   challenge_1 = H(the body of section 1), for a file without records
 *   pub(c) = U of the five after-values, then of the nine key points, in record order (1216 bytes)
 *   challenge_{k+1} = H(challenge_k || pub(c_k)): the record's nextChallenge, and the hash a participant publishes
 *   for the secret x_j, j = 0 (tau), 1 (alpha), 2 (beta), and a random s_j:
 *     g1_s = s_j G1      g1_sx = x_j g1_s      g2_sp = hash_to_g2(H(challenge_k || u8(j) || U1(g1_s) || U1(g1_sx)))      g2_spx = x_j g2_sp
 * Compatibility.  The transcript is this library's own, as phase 2's is: records made here are not accepted by `snarkjs
 * powersoftau verify`, and records made by snarkjs are not accepted here.  Sections 1 to 6 of a contributed file are ordinary.
 *
 * Where the work runs.  gwb_ptau_new, the nine single-point multiplications of a record, betaG2 and hash_to_g2 run on the host.
 * The 5 2^P - 1 G1 points and 2^P G2 points of sections 2 to 5 go through the device in pieces of CWC_CONTRIBUTE_CHUNK points
 * (environment, default 2^18): one kernel makes the piece's scalars c tau'^(first + i) from a table of tau'^(2^b) in device
 * memory, one decodes, checks (coordinates, curve: the messages of the setup) and multiplies each point by its scalar
 * (r1cs/ceremony.hip: signed windows of 3 bits with the table of multiples in LDS), the shared-inversion kernel of the setups
 * writes the stored bytes.
 *
 * Return convention: that of graph_witness_groth16_contribute.h's verifications: 0; 1 when a file was read and a rule of a
 * verification failed; 2 for every other failure (bytes that are no file, a secret outside [1, r), a device error). */
#ifndef CWC_AMD_GRAPH_WITNESS_GROTH16_CEREMONY_H
#define CWC_AMD_GRAPH_WITNESS_GROTH16_CEREMONY_H

#include <stddef.h>
#include <stdint.h>

#include "graph_witness_groth16_contribute.h"
#include "graph_witness_groth16_ptau.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A new ceremony file of the given power, 1 <= power <= 28, ceremonyPower = power: sections 1 to 7 in ascending order, every
 * point its group's generator, section 7 = u32 0.  Host only.  *out is freed with gwb_groth16_setup_free; an allocation that
 * fails is refused with a message naming the bytes. */
int gwb_ptau_new(uint32_t power, void **out, size_t *out_len, gw_status_t *status);

/* One contribution to the file `ptau` (header, section table and section 7 parsed and everything sized before the device is
 * touched).  name: at most 255 bytes, may be NULL or empty.  secrets: 96 bytes, tau', alpha', beta', each canonical
 * little-endian in [1, r), or NULL to draw them from getrandom().  out: the new file, freed with gwb_groth16_setup_free; hash64:
 * the new record's nextChallenge.  Synchronous, on the current device. */
int gwb_ptau_contribute(const void *ptau, size_t len, const char *name, const uint8_t *secrets, void **out, size_t *out_len, void *hash64,
                        gw_status_t *status);
/* {load, scalars, mul_g1, mul_g2, affine} in ms of the process's last gwb_ptau_contribute call, summed over its pieces; 1 when
 * there is none. */
int gwb_ptau_contribute_phase_ms(float *ms);

/* Verifies a ceremony file: its records, and that the whole file is what its sections say.  The rules, in this order; the first
 * that fails is the message:
 *   1. The file parses: header, section table, section 7 as above, and every point of sections 2 to 6 has coordinates below q
 *      and lies on its curve (host; returns 2 with the loader's messages).  Before the device is touched.
 *   2. Unless GWB_PTAU_VERIFY_SKIP_RECORDS, every record, with prev = the previous record's after-values, or the generators for
 *      the first record: nextChallenge is as recomputed from the challenge before it; no point is at infinity; the three g2_spx,
 *      tauG2 and betaG2 are in the order-r subgroup (host, the criterion of r1cs/g2_subgroup_gfx950.hpp);
 *      e(g1_s, g2_spx) = e(g1_sx, g2_sp) for each secret; e(after, g2_sp) = e(prev, g2_spx) for tauG1, alphaG1 and betaG1;
 *      e(tauG1, G2) = e(G1, tauG2); e(betaG1, G2) = e(G1, betaG2).  Then the last record's after-values are the file's tauG1[1],
 *      tauG2[1], alphaTauG1[0], betaTauG1[0] and betaG2; without records these are the generators.
 *      Example: "ptau: contribution 2: alphaG1 is not the previous alphaG1 times the proven secret".
 *   3. The whole-file powers check: every point of section 3 is in the order-r subgroup (device); then the six sums and five
 *      equations of gwb_ptau_check_powers (graph_witness_groth16_ptau.h) over the whole file: V and U over the 2^(power+1) - 2
 *      pairs of neighbours of section 2, so that its last point is read, and 2^power points of sections 3 to 5.  The messages
 *      say "the points" where that function says "the first n points".
 * All pairings of rules 2 and 3 run in one batched launch.  With GWB_PTAU_VERIFY_SKIP_RECORDS rules 1 and 3 alone run: that is
 * for files that carry snarkjs's records, which this library cannot verify by design; then nothing shows who made the file's
 * tau, alpha and beta.  NOT verified: sections 12 to 15 (gwb_ptau_check_lagrange does that); records made by snarkjs.
 * seed: 32 bytes for the rho of rule 3, or NULL to draw them.  hashes_out: room for *n hashes of 64 bytes (may be NULL with
 * *n = 0); *n returns the number of records, and the first min(*n in, *n out) of their nextChallenge values are written, oldest
 * first, on success.  Returns 0; 1 when a rule failed, with a message that names the record and the rule or the section; 2
 * otherwise.  Synchronous, on the current device. */
#define GWB_PTAU_VERIFY_SKIP_RECORDS 1u
int gwb_ptau_verify(const void *ptau, size_t len, uint32_t flags, const uint8_t *seed, void *hashes_out, size_t *n, gw_status_t *status);

/* Checks that `next` is `prev` after exactly one contribution: section 1 is identical; `next` has exactly one record more and the
 * earlier ones are byte-identical; the new record passes the rules of 2. above with prev = tauG1[1], tauG2[1], alphaTauG1[0],
 * betaTauG1[0] and betaG2 read from the previous FILE and the challenge before it = the previous file's last nextChallenge as
 * stored (H(section 1) without records), so the check also works on top of records this library cannot verify; the record's
 * after-values are `next`'s points; the whole-file check 3. of `next` runs last.  No linear combination across the two files
 * is needed: once the five anchor points are tied to the previous file by the record, the powers check fixes every other
 * point.  Returns as gwb_ptau_verify. */
int gwb_ptau_verify_step(const void *prev, size_t prev_len, const void *next, size_t next_len, const uint8_t *seed, gw_status_t *status);

/* Host only.  The records of a file's section 7 as a flat image (freed with gwb_groth16_setup_free): u32 n, then per record the
 * five after-values and the nine key points in record order, canonical little-endian as the C ABI's points (1216 B),
 * nextChallenge (64 B), u32 type, u32 nameLen, name.  Nothing is verified beyond the section's form. */
int gwb_ptau_contributions(const void *ptau, size_t len, void **out, size_t *out_len, gw_status_t *status);

/* Measurement and test aids of the multiplication kernel: d_out[i] = d_scalars[i] d_points[i].  Device points in `form`
 * (GWB_FORM_CANONICAL or GWB_FORM_MONTGOMERY of graph_witness_batch.h; G1 64 B, G2 128 B x.c0, x.c1, y.c0, y.c1; zero bytes =
 * infinity, which stays; not validated), d_scalars [n][32 B] canonical little-endian below r, d_out the products in the same
 * form.  method: the windowed kernel or xyzz_mul_short per thread.  Asynchronous on hip_stream (the workspace is allocated and
 * freed in stream order). */
#define GWB_MUL_WINDOW 0u
#define GWB_MUL_PLAIN 1u
int gwb_bn254_g1_mul_batch_device(const void *d_points, const void *d_scalars, size_t n, uint32_t form, uint32_t method, void *d_out,
                                  void *hip_stream, gw_status_t *status);
int gwb_bn254_g2_mul_batch_device(const void *d_points, const void *d_scalars, size_t n, uint32_t form, uint32_t method, void *d_out,
                                  void *hip_stream, gw_status_t *status);

#ifdef __cplusplus
}
#endif
#endif /* CWC_AMD_GRAPH_WITNESS_GROTH16_CEREMONY_H */
