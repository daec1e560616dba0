/* Groth16 phase-2 contributions on an MI355X: what snarkjs `zkey contribute` and `zkey verify` do to a key's delta, with this
 * library's own challenge derivation (below: the records are NOT interchangeable with snarkjs's).
 *
 * A contribution with secret d does four things to a `.zkey`: delta1 and delta2 are multiplied by d; every point of sections
 * 8 (C) and 9 (H) is multiplied by 1 / d; everything else stays byte for byte; a record with a proof of knowledge of d is
 * appended to section 10.  A key made from a powers-of-tau file with delta = 1 (gwb_groth16_setup_ptau) and contributed to
 * with d1, d2, ... holds in sections 1 to 9 exactly the bytes of the trapdoor setup with delta = d1 d2 ... mod r.
 *
 * Trust.  After contributions by several parties the key's delta is known to nobody unless ALL of them kept and pooled their
 * secrets; one honest participant who discarded d is enough.  Each call draws d (unless given), and zeroes d, 1 / d and the
 * nonce s on the host and on the device before it returns.  A d passed in by the caller is the caller's to discard.
 *
 * Section 10 (snarkjs's writeMPCParams, restated; points affine, Montgomery, little-endian as everywhere in the file):
 *   64 B csHash | u32 nContributions | per record:
 *     deltaAfter G1 64 B | g1_s G1 64 B | g1_sx G1 64 B | g2_spx G2 128 B | transcript 64 B
 *     u32 type (0 = contribution, 1 = beacon) | u32 paramsLen | params
 *   params: tagged items  01 len name[len]  |  02 numIterationsExp  |  03 len beaconHash[len]
 * Records of type 1 are made by gwb_groth16_beacon and checked against their parameters by the verifications below
 * (graph_witness_groth16_beacon.h); a contribution carries them byte for byte.  The reader refuses, with a message that starts
 * "zkey: section 10": a truncated section, a record count the section cannot hold, a paramsLen or an item length that runs
 * past its end, an unknown tag or type, a coordinate >= q, a point off its curve, trailing bytes.
 *
 * Transcript and challenge.  H is unkeyed BLAKE2b-512 (RFC 7693).
 *   U1(P)  = x || y, 32 bytes each, canonical, big-endian (G1)
 *   U2(P)  = x.c1 || x.c0 || y.c1 || y.c0, likewise (G2)
 *   pub(c) = U1(deltaAfter) || U1(g1_s) || U1(g1_sx) || U2(g2_spx) || transcript
 *   transcript_k = H(csHash || pub(c_1) || ... || pub(c_{k-1}) || U1(g1_s_k) || U1(g1_sx_k))
 *   hash_k = H(pub(c_k)): what a participant publishes
 *   g2_sp_k = hash_to_g2(transcript_k)
 * hash_to_g2(t) tries ctr = 0, 1, ... and returns the first point: d = H(t || "cwc-g2" || u32le(ctr)); c0 = the little-endian
 * integer of d[0:32] with its top two bits cleared, c1 likewise from d[32:64]; next ctr if c0 >= q or c1 >= q; x = c0 + c1 u;
 * next ctr if x^3 + 3 / (9 + u) is not a square in Fq2; y = the root whose canonical pair (c1, c0) is the smaller of the two;
 * P = (2q - r) (x, y); next ctr if P = O; P in affine form.  (The square root runs on the host by the norm method, q = 3 mod 4.)
 * A record proves knowledge of d by g1_sx = d g1_s for a random g1_s = s G1 and g2_spx = d g2_sp.
 *
 * Compatibility.  The record layout and the encodings U1, U2 follow snarkjs as read from its source.  The challenge
 * derivation hash_to_g2 is this library's own: snarkjs derives its point from a ChaCha stream seeded with the transcript,
 * which cannot be restated faithfully here.  So records made here are not accepted by `snarkjs zkey verify`, and records
 * made by snarkjs are not accepted here.  Sections 1 to 9 of a contributed key are ordinary: snarkjs, rapidsnark and this
 * library prove and verify with it.  The derivation lives in one function (r1cs/contributions.cc, hash_to_g2).
 *
 * csHash: if the incoming key has no records and an all-zero csHash (the state the setups write), the first contribution
 * sets csHash = H(the bodies of sections 1 to 9 of the incoming key, in id order); otherwise csHash is carried unchanged.
 *
 * Where the work runs.  The five single-point multiplications of a contribution (g1_s, g1_sx, g2_spx, delta1, delta2) and
 * hash_to_g2 run on the host.  Sections 8 and 9, one list of (nVars - nPublic - 1) + domainSize points, go to the device in
 * pieces of CWC_CONTRIBUTE_CHUNK points (environment, default 2^18): one kernel decodes each point and multiplies it by the
 * wave-uniform scalar 1 / d, the shared-inversion kernel of the setups writes the stored bytes; infinity stays zero bytes.
 * The subgroup checks of the few G2 points of a verification run on the host (the criterion of r1cs/g2_subgroup_gfx950.hpp);
 * all pairings of a verification go through the device pairing in one batched launch and their 384-byte values are
 * compared on the host.
 *
 * Return and status conventions are those of graph_witness_r1cs.h, with one addition: the two verification functions return
 * 1 when the key was read and a rule failed (status names the first failing record and rule), and 2 for every other failure
 * (bytes that are no key, a device error).  gwb_zkey_verify_key follows them too. */
#ifndef CWC_AMD_GRAPH_WITNESS_GROTH16_CONTRIBUTE_H
#define CWC_AMD_GRAPH_WITNESS_GROTH16_CONTRIBUTE_H

#include <stddef.h>
#include <stdint.h>

#include "graph_witness_groth16.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GWB_CONTRIBUTION_HASH_BYTES 64
#define GWB_CONTRIBUTION_NAME_MAX 255

/* One contribution to the key `zkey` (parsed and checked as gwb_zkey_load does, section 10 as above, before the device is
 * touched).  name: at most 255 bytes, may be NULL or empty.  delta: 32 bytes, canonical little-endian, in [1, r), or NULL to
 * draw it from getrandom().  out: the new key (sections 1 to 10 in ascending order), freed with gwb_groth16_setup_free;
 * hash64: hash_k of the new record.  Synchronous, on the current device. */
int gwb_groth16_contribute(const void *zkey, size_t len, const char *name, const uint8_t *delta, void **out, size_t *out_len,
                           void *hash64, gw_status_t *status);
/* {load, scale, affine} in ms of the process's last gwb_groth16_contribute call, summed over its pieces; 1 when there is none. */
int gwb_groth16_contribute_phase_ms(float *ms);

/* Checks the records of a key.  With deltaPrev = G1 for the first record and deltaAfter_{k-1} afterwards, every record needs:
 * its transcript as recomputed; no point at infinity; g2_spx in the order-r subgroup; e(g1_s, g2_spx) = e(g1_sx, g2_sp);
 * e(deltaPrev, g2_spx) = e(deltaAfter, g2_sp).  At the end: deltaAfter_last = the header's delta1 (delta1 = G1 without
 * records); delta2 in the subgroup; e(delta1, G2) = e(G1, delta2).  hashes_out: room for *n hashes of 64 bytes (may be NULL
 * with *n = 0); *n returns the number of records, and the first min(*n in, *n out) hashes are written.
 * Example of a refusal: "zkey: contribution 2: deltaAfter is not deltaPrev times the proven secret". */
int gwb_zkey_verify_contributions(const void *zkey, size_t len, void *hashes_out, size_t *n, gw_status_t *status);

/* Checks that `next` is `prev` after exactly one contribution: one record more, the earlier ones byte-identical; csHash
 * carried, or H(sections 1 to 9 of prev) where prev is blank; sections 1, 3, 4, 5, 6, 7 and alpha1, beta1, beta2, gamma2
 * identical; the new record passes the rules above with deltaPrev = prev's delta1; and, with P = prev's C || H, P' = next's
 * and 128-bit rho_i, R = sum rho_i P_i and R' = sum rho_i P'_i computed on the device, per section,
 * e(R', delta2') = e(R, delta2).  rho is cut four per digest from H(seed || u64le(j)), j = i / 4 over the joint index of
 * C || H; seed: 32 bytes, or NULL to draw them from getrandom().  A key whose C or H differs from the honest one in any
 * point is accepted with probability about 2^-128 over the seed, so a verifier draws the seed after it has seen the key. */
int gwb_zkey_verify_step(const void *prev, size_t prev_len, const void *next, size_t next_len, const uint8_t *seed, gw_status_t *status);

/* Checks that `zkey` is the honest key of the circuit `r` and the powers-of-tau file `ptau`, with a delta that only the recorded
 * contributions touched: what `snarkjs zkey verify circuit.r1cs pot.ptau key.zkey` answers.  The rules, in this order; the first
 * failure is the message:
 *   1. Parse.  The key parses as for the functions above; the file passes the loader's checks of graph_witness_groth16_ptau.h
 *      for the circuit's domain under lagrange_mode (returns 2 with their messages).
 *   2. Sizes.  nVars, nPublic and domainSize of the key are the circuit's ("zkey verify: nVars of the key is 7, the circuit's
 *      is 9").  Everything up to here runs before the device is touched.
 *   3. With GWB_VERIFY_KEY_CHECK_PTAU: gwb_ptau_check_powers for the circuit's domain power, with its messages ("ptau: ...").
 *   4. Remake.  key0 = gwb_groth16_setup_ptau(r, ptau, delta = 1, lagrange_mode) (a failure returns 2 with its message).
 *      GWB_PTAU_LAGRANGE_COMPUTE keeps the verdict off the file's sections 12 to 15, which nothing verifies.
 *   5. Structure.  Section 4 agrees with the circuit by gwb_zkey_check_r1cs's rule (not by bytes); sections 1, 3, 5, 6, 7 and
 *      the header before delta1 (the sizes, alpha1, beta1, beta2, gamma2) are key0's byte for byte ("zkey verify: section 5 (A)
 *      differs from the key remade from the circuit and the powers-of-tau file").
 *   6. Records, unless GWB_VERIFY_KEY_SKIP_RECORDS: the csHash is blank (only without records) or H(sections 1 to 9 of key0);
 *      then every rule of gwb_zkey_verify_contributions, so without records delta1 and delta2 are the generators.
 *   7. delta, always: neither delta point at infinity, delta2 in the order-r subgroup, e(delta1, G2) = e(G1, delta2).
 *   8. C and H: with the 128-bit rho of gwb_zkey_verify_step over key0's and the key's C || H, per section
 *      e(R', delta2) = e(R, G2); a sum at infinity on one side only is a failure ("zkey verify: section 8 (C) is not the remade
 *      key's section divided by delta").
 * All pairings of rules 6 to 8 run in one batched launch.  A verdict of a rule shared with gwb_zkey_verify_contributions reads
 * "zkey verify: ..." where that function says "zkey: ...".  GWB_VERIFY_KEY_SKIP_RECORDS is for keys that carry snarkjs's
 * records, which this library cannot verify by design: their points are still checked against circuit, file and their own
 * delta, but then nothing shows who made that delta.
 * NOT verified: records made by snarkjs in the `.ptau` (gwb_ptau_verify of graph_witness_groth16_ceremony.h checks this
 * library's); the file's points beyond the prefixes a setup reads (the same function checks the whole file);
 * sections 12 to 15 of the file, on which the verdict rests unless lagrange_mode is GWB_PTAU_LAGRANGE_COMPUTE; records made by
 * snarkjs.  seed: 32 bytes for rho (here and in rule 3), or NULL to draw them.  hashes_out and *n as for
 * gwb_zkey_verify_contributions, filled on success.  Returns 0; 1 when a rule failed, with a message that starts
 * "zkey verify:" or "ptau:"; 2 otherwise.  Synchronous, on the current device. */
#define GWB_VERIFY_KEY_SKIP_RECORDS 1u
#define GWB_VERIFY_KEY_CHECK_PTAU 2u
int gwb_zkey_verify_key(const void *zkey, size_t len, gwb_r1cs_t *r, const void *ptau, size_t ptau_len, uint32_t lagrange_mode,
                        uint32_t flags, const uint8_t *seed, void *hashes_out, size_t *n, gw_status_t *status);
/* {remake, linear combinations, pairings} in ms of the process's last accepted gwb_zkey_verify_key call (host clock around the
 * three synchronous parts; the powers check of rule 3 is in none of them); 1 when there is none. */
int gwb_zkey_verify_key_phase_ms(float *ms);

/* Host-only aids.  The records of a key's section 10 as a flat image (freed with gwb_groth16_setup_free): 64 B csHash, u32 n,
 * then per record deltaAfter, g1_s, g1_sx (64 B each), g2_spx (128 B), canonical little-endian as the C ABI's points,
 * transcript (64 B), hash (64 B), u32 type, u32 nameLen, name. */
int gwb_zkey_contributions(const void *zkey, size_t len, void **out, size_t *out_len, gw_status_t *status);
void gwb_blake2b512(const void *data, size_t len, void *out64);
/* hash_to_g2 of a 64-byte transcript: 128 bytes, canonical little-endian x.c0, x.c1, y.c0, y.c1 */
void gwb_zkey_contribution_challenge(const void *t64, void *out128);

/* Measurement and test aids of the two kernels; canonical affine device points (64 B, zero bytes = infinity, not validated),
 * asynchronous on hip_stream (workspaces allocated and freed in stream order).
 * d_out[i] = k d_points[i] for the one canonical scalar k32 (32 bytes, host memory, read before the call returns). */
int gwb_bn254_g1_scale_batch_device(const void *d_points, size_t n, const uint8_t *k32, void *d_out, void *hip_stream, gw_status_t *status);
/* *d_out (one point) = sum_i rho_i d_points[i], d_rho device [n][16] little-endian */
int gwb_bn254_g1_lincomb128_device(const void *d_points, const void *d_rho, size_t n, void *d_out, void *hip_stream, gw_status_t *status);
/* the same in G2: points of 128 B (x.c0, x.c1, y.c0, y.c1), one point of 128 B out */
int gwb_bn254_g2_lincomb128_device(const void *d_points, const void *d_rho, size_t n, void *d_out, void *hip_stream, gw_status_t *status);

#ifdef __cplusplus
}
#endif
#endif /* CWC_AMD_GRAPH_WITNESS_GROTH16_CONTRIBUTE_H */
