/* A random beacon closes a ceremony phase on an MI355X: what snarkjs `powersoftau beacon` and `zkey beacon` do, with this library's
 * own derivation (below: as with its transcripts, the records are NOT interchangeable with snarkjs's, which derives its keys from
 * a ChaCha stream).
 *
 * Why.  A ceremony that ends on an ordinary contribution lets its last participant choose their secret after seeing everybody
 * else's.  A beacon is a last contribution whose secrets nobody chooses: they are derived by a public, deliberately slow hash
 * chain from a value that did not exist when the last participant contributed (a block hash, a drand round).  Anybody can
 * recompute them, so a beacon adds no secrecy; it removes the last participant's choice.
 *
 * The derivation.  beaconHash: 1 to 255 bytes.  numIterationsExp = e, 10 <= e <= 63 (snarkjs's range).
 *   D_0 = beaconHash      D_{i+1} = SHA-256(D_i) for i < 2^e      D = D_{2^e} (32 bytes)
 *   scalar(phase, j) = the first nonzero value, over ctr = 0, 1, ..., of
 *                      (the big-endian integer of BLAKE2b-512("cwc-beacon" || u8(phase) || D || u8(j) || u32le(ctr))) mod r
 *   phase 1 (`.ptau`): j = 0, 1, 2 are tau', alpha', beta'; j = 3, 4, 5 are the nonces s_0, s_1, s_2 of the three proofs of knowledge
 *   phase 2 (`.zkey`): j = 0 is delta'; j = 1 is the nonce s
 * A beacon record is the record of a contribution with these secrets and nonces, with type = 1 and the parameters
 *   01 len name[len] (omitted when the name is empty) | 02 e | 03 len beaconHash[len]
 * in this order; in a `.ptau` its partialHash is zeros.  The whole output is therefore a function of the incoming file, the
 * name, beaconHash and e: two runs give identical bytes.  The secrets are public, so there is nothing to zero, and nothing
 * is lost when they are printed (gwb_beacon_scalars).
 *
 * The limit.  The chain is sequential and runs on the host, in making and in verifying.  A hostile file could state e = 63 and
 * hang a verifier, so both refuse an e above CWC_BEACON_MAX_EXP (environment, read once per process; a decimal number in
 * [10, 63], anything else and unset: 28).  The refusal returns 2, it is no verdict about the file:
 *   "ptau: contribution 3: numIterationsExp 40 is above the limit 28 (CWC_BEACON_MAX_EXP)"      ("zkey: ..." for a key)
 *   "beacon: numIterationsExp 40 is above the limit 28 (CWC_BEACON_MAX_EXP)"                    (the making calls)
 *
 * Verifying.  In gwb_ptau_verify, gwb_ptau_verify_step, gwb_zkey_verify_contributions, gwb_zkey_verify_step and
 * gwb_zkey_verify_key a record of type 1 passes every rule of its kind and additionally the beacon rule:
 *   form   its parameters hold exactly one item 02 and one item 03, with a hash of 1 to 255 bytes, and e is in [10, 63] (returns 1)
 *          and at most the limit (returns 2).  This needs the parsed section alone and runs right after the file parses, before
 *          the device is touched:  "ptau: contribution 3: a beacon record needs numIterationsExp and beaconHash"
 *   key    for each secret, g1_s = s_j G1 and g1_sx = x_j g1_s are the record's points, with (x_j, s_j) recomputed from the
 *          parameters.  With the pairing rules this fixes g2_spx and the after-values.  Host, after the record's other host rules
 *          and before the batched pairing launch:
 *            "ptau: contribution 3: the key of secret alpha is not the one its beaconHash and numIterationsExp give"
 *            "zkey: contribution 3: the key is not the one its beaconHash and numIterationsExp give"   ("zkey verify: ..." in
 *            gwb_zkey_verify_key)
 * The functions that pass over the records on request (GWB_PTAU_VERIFY_SKIP_RECORDS, GWB_VERIFY_KEY_SKIP_RECORDS) pass over this
 * rule too.  A record of type 1 whose key is not derived from its parameters, for instance one made by snarkjs, is refused;
 * before this rule existed it was checked as an ordinary contribution.  Whether the LAST record is a beacon is not a rule of
 * these functions: a caller who requires it reads the record list (the Python wrappers' require_beacon, the CLIs'
 * --require-beacon).
 *
 * Where the work runs.  SHA-256, the chain, the derivation and the single-point multiplications of a record run on the host.
 * The points of the file or key go through the device exactly as for a contribution, through the same internal path with
 * (secrets, nonces, type, parameters): phase 1 through fr_scalars_kernel and mul_points_kernel (r1cs/ceremony.hip), phase 2
 * through the wave-uniform scale kernel (r1cs/contribute.hip), both through the shared-inversion kernel of the setups.
 * gwb_ptau_contribute_phase_ms and gwb_groth16_contribute_phase_ms report a beacon call like a contribution.
 *
 * Return convention: 0, or 2 with a message; the functions here give no verdicts. */
#ifndef CWC_AMD_GRAPH_WITNESS_GROTH16_BEACON_H
#define CWC_AMD_GRAPH_WITNESS_GROTH16_BEACON_H

#include <stddef.h>
#include <stdint.h>

#include "graph_witness_groth16_ceremony.h"
#include "graph_witness_groth16_contribute.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GWB_BEACON_EXP_MIN 10u
#define GWB_BEACON_EXP_MAX 63u
#define GWB_BEACON_HASH_MAX 255

/* The beacon of phase 1 on the file `ptau`: exactly what gwb_ptau_contribute gives for the derived secrets, except that the
 * nonces are the derived ones, the record's type is 1 and its parameters are the beacon's; sections 12 to 15 are dropped and
 * unknown sections carried as there.  Refused before the device is touched, with a message that starts "beacon:": e outside
 * [10, 63] or above the limit, an empty hash or one above 255 bytes, a name above 255 bytes; and everything gwb_ptau_contribute
 * refuses about the file.  out: the new file, freed with gwb_groth16_setup_free; hash64: the record's nextChallenge. */
int gwb_ptau_beacon(const void *ptau, size_t len, const char *name, const void *beacon_hash, size_t hash_len, uint32_t iterations_exp,
                    void **out, size_t *out_len, void *hash64, gw_status_t *status);

/* The beacon of phase 2 on the key `zkey`: the same relation to gwb_groth16_contribute, the csHash rule for a blank key
 * included.  hash64: hash_k of the new record. */
int gwb_groth16_beacon(const void *zkey, size_t len, const char *name, const void *beacon_hash, size_t hash_len, uint32_t iterations_exp,
                       void **out, size_t *out_len, void *hash64, gw_status_t *status);

/* Host only, for audit and tests: the scalars of a beacon, 6 (phase 1) or 2 (phase 2) times 32 bytes, canonical little-endian,
 * in the order above.  Returns 2 without writing for a phase other than 1 or 2 and for arguments the making calls refuse. */
int gwb_beacon_scalars(uint32_t phase, const void *beacon_hash, size_t hash_len, uint32_t iterations_exp, void *out);

/* Host only.  The raw parameter bytes (the tagged items) of record k, 0-based, of a file's section 7 or a key's section 10, freed
 * with gwb_groth16_setup_free; *out_len may be 0.  The flat images of gwb_ptau_contributions and gwb_zkey_contributions keep
 * their layout and carry the name alone. */
int gwb_ptau_contribution_params(const void *ptau, size_t len, size_t k, void **out, size_t *out_len, gw_status_t *status);
int gwb_zkey_contribution_params(const void *zkey, size_t len, size_t k, void **out, size_t *out_len, gw_status_t *status);

/* SHA-256 (FIPS 180-4) of `len` bytes, an aid beside gwb_blake2b512: the chain's link. */
void gwb_sha256(const void *data, size_t len, void *out32);

#ifdef __cplusplus
}
#endif
#endif /* CWC_AMD_GRAPH_WITNESS_GROTH16_BEACON_H */
