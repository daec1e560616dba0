// Section 10 of a `.zkey` (the phase-2 contribution records), BLAKE2b-512, the transcript and the challenge point, as
// include/graph_witness_groth16_contribute.h defines them: contributions.cc (host only), shared with contribute.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "bn254_points_gfx950.hpp"
#include "groth16_internal.hpp"
#include "ptau_internal.hpp"

namespace cwc_contrib {

constexpr size_t HASH_BYTES = 64;
constexpr size_t PUB_BYTES = 3 * G1_BYTES + G2_BYTES + HASH_BYTES;  // pub(c): U1, U1, U1, U2, transcript
constexpr size_t RECORD_FIXED_BYTES = PUB_BYTES + 8;                 // the points, the transcript, u32 type, u32 paramsLen

// Unkeyed BLAKE2b with a 64-byte digest (RFC 7693), incremental.
class Blake2b {
    uint64_t h_[8], t_ = 0;
    uint8_t buf_[128];
    size_t fill_ = 0;
    void compress(const uint8_t* block, bool last);

public:
    Blake2b();
    void update(const void* data, size_t len);
    void final(uint8_t out[HASH_BYTES]);
};
void blake2b512(const void* data, size_t len, uint8_t out[HASH_BYTES]);

// One record; the points as the file stores them (affine, Montgomery, little-endian).
struct Record {
    uint8_t delta_after[G1_BYTES], g1_s[G1_BYTES], g1_sx[G1_BYTES], g2_spx[G2_BYTES], transcript[HASH_BYTES];
    uint32_t type = 0;            // 0 = contribution, 1 = beacon (beacon.hpp)
    std::vector<uint8_t> params;  // the tagged items, byte for byte
    std::string name;             // item 01 of params, if there is one
};
struct Section10 {
    uint8_t cs_hash[HASH_BYTES] = {};
    std::vector<Record> recs;
    bool blank() const;  // no records and an all-zero csHash: the state the setups write
};

// Hostile bytes in; every refusal starts "zkey: section 10".
bool parse_section10(const uint8_t* p, uint64_t size, Section10& out, std::string& err);
void write_section10(const Section10& s, std::vector<uint8_t>& out);
std::vector<uint8_t> name_params(const std::string& name);  // item 01 for a name of at most 255 bytes ("" gives no item)

// U1 / U2: canonical big-endian coordinates of a stored point (64 or 128 bytes out)
void u1_bytes(const uint8_t* stored, uint8_t* out);
void u2_bytes(const uint8_t* stored, uint8_t* out);
void pub_bytes(const Record& r, uint8_t out[PUB_BYTES]);
void record_hash(const Record& r, uint8_t out[HASH_BYTES]);
// transcript_k for the record with index k (0-based) of s, from the records before it and from g1_s, g1_sx (stored form)
void transcript_of(const Section10& s, size_t k, const uint8_t* g1_s, const uint8_t* g1_sx, uint8_t out[HASH_BYTES]);
// The challenge point of a transcript, Montgomery affine.  The one place that derives it.
cwc_g16::A2 hash_to_g2(const uint8_t t[HASH_BYTES]);

// k P on the host for a canonical k, stored bytes in and out
void g1_mul_stored(const uint8_t* in, const cwc::Fr& k, uint8_t* out);
void g2_mul_stored(const uint8_t* in, const cwc::Fr& k, uint8_t* out);
void put_stored(uint8_t* out, const cwc_g16::A1& p);
void put_stored(uint8_t* out, const cwc_g16::A2& p);
bool g2_stored_in_subgroup(const uint8_t* in);  // on the twist already; the criterion of g2_subgroup_gfx950.hpp
// canonical little-endian bytes of a stored point, the C ABI's form (for the pairing and for the record dump)
void canonical_g1(const uint8_t* stored, uint8_t* out);
void canonical_g2(const uint8_t* stored, uint8_t* out);

// ---- contribute.hip's checks, shared with the ceremony's verification (ceremony.hip) ---------------------------------------------

// e(a1, a2) = e(b1, b2)?  Stored points; `msg` is what the failure says.
struct PairCheck {
    const uint8_t *a1, *a2, *b1, *b2;
    std::string msg;
};
// Runs the pairings of `checks` in one batched launch; verdict = the message of the first check that fails, "" if none does.
bool run_pair_checks(const std::vector<PairCheck>& checks, std::string& verdict, std::string& err);
// the caller's 32 bytes, or without them 32 from getrandom()
bool seed_or_draw(const uint8_t* in, uint8_t seed[32]);
// The six sums of the powers check and the generators, stored form: what its five equations point into.
struct PowersSums {
    uint8_t g1[5 * G1_BYTES], s2[G2_BYTES], gen1[G1_BYTES], gen2[G2_BYTES];
};

// The six sums over the first n points of sections 3 to 5 and the first `pairs` points of section 2 with the point after each, and
// the five equations of the powers check (graph_witness_groth16_ptau.h) into `checks`; `keep` has to outlive them.  whole: the
// lengths are a whole file's and the messages say "the points".  host_verdict: the first equation that fails without a pairing.
bool powers_rules(const cwc_ptau::Plan& pl, uint64_t n, uint64_t pairs, bool whole, const uint8_t seed[32], PowersSums& keep, std::vector<PairCheck>& checks,
                  std::string& host_verdict, std::string& err);

}  // namespace cwc_contrib
