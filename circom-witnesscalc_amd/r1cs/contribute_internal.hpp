// Section 10 of a `.zkey` (the phase-2 contribution records), BLAKE2b-512, the transcript and the challenge point, as
// include/graph_witness_groth16_contribute.h defines them: contributions.cc (host only), shared with contribute.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "bn254_points_gfx950.hpp"
#include "groth16_internal.hpp"

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
    uint32_t type = 0;            // 0 = contribution, 1 = beacon (kept, never made here)
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

}  // namespace cwc_contrib
