// Section 7 of a `.ptau` (the ceremony's contribution records), the ceremony's transcript and the image of a contributed file,
// as include/graph_witness_groth16_ceremony.h defines them: ceremony.cc (host only), shared with ceremony.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "bn254_points_gfx950.hpp"
#include "contribute_internal.hpp"
#include "groth16_internal.hpp"
#include "ptau_internal.hpp"
#include "r1cs_internal.hpp"

namespace cwc_ceremony {

using cwc_contrib::HASH_BYTES;

constexpr uint32_t POW_BITS = 30;  // the index of a point in its section is below 2^29 (power 28, section 2)
constexpr size_t PARTIAL_HASH_BYTES = 216;
constexpr size_t AFTER_BYTES = 3 * G1_BYTES + 2 * G2_BYTES;                                  // tauG1, tauG2, alphaG1, betaG1, betaG2
constexpr size_t KEY_BYTES = 6 * G1_BYTES + 3 * G2_BYTES;                                    // g1_s, g1_sx per secret, then the three g2_spx
constexpr size_t RECORD_FIXED_BYTES = AFTER_BYTES + KEY_BYTES + PARTIAL_HASH_BYTES + HASH_BYTES + 8;  // ..., u32 type, u32 paramsLen
constexpr size_t PUB_BYTES = AFTER_BYTES + KEY_BYTES;                                        // U1 and U2 are as long as the stored points

// One record; the points as the file stores them (affine, Montgomery, little-endian).  Secret j is tau (0), alpha (1), beta (2).
struct PtauRecord {
    uint8_t tau_g1[G1_BYTES], tau_g2[G2_BYTES], alpha_g1[G1_BYTES], beta_g1[G1_BYTES], beta_g2[G2_BYTES];  // the after-values
    uint8_t g1_s[3][G1_BYTES], g1_sx[3][G1_BYTES], g2_spx[3][G2_BYTES];
    uint8_t partial_hash[PARTIAL_HASH_BYTES] = {};  // snarkjs's saved hash state: zeros here, kept byte for byte in foreign records
    uint8_t next_challenge[HASH_BYTES];
    uint32_t type = 0;            // 0 = contribution, 1 = beacon (beacon.hpp)
    std::vector<uint8_t> params;  // the tagged items, byte for byte
    std::string name;             // item 01 of params, if there is one
};
struct Section7 {
    std::vector<PtauRecord> recs;
};

// Hostile bytes in; every refusal starts "ptau: section 7".  p == nullptr (a file without the section): no records.
bool parse_section7(const uint8_t* p, uint64_t size, Section7& out, std::string& err);
void write_section7(const Section7& s, std::vector<uint8_t>& out);

// pub(c): U of the five after-values, then of the nine key points, in record order
void pub_bytes(const PtauRecord& r, uint8_t out[PUB_BYTES]);
// challenge_{k+1} = H(challenge_k || pub(c_k))
void next_challenge(const uint8_t challenge[HASH_BYTES], const PtauRecord& r, uint8_t out[HASH_BYTES]);
// The challenge before the record with index k (0-based): H(body of section 1) for k = 0, else the nextChallenge that record k - 1
// states.
void last_challenge(const uint8_t* sec1, uint64_t sec1_size, const Section7& s, size_t k, uint8_t out[HASH_BYTES]);
// g2_sp of secret j: hash_to_g2(H(challenge || u8(j) || U1(g1_s) || U1(g1_sx))), Montgomery affine
cwc_g16::A2 key_challenge_point(const uint8_t challenge[HASH_BYTES], uint32_t j, const uint8_t* g1_s, const uint8_t* g1_sx);

// The file after a contribution: the input's sections in the input's order with sections 2 to 6 replaced by bodies[0 .. 5)
// (their sizes are the input's) and section 7 by `s`, sections 12 to 15 dropped, every other section byte for byte; a file
// without section 7 gets one at the end.  *out is freed with gwb_groth16_setup_free.  0, or 2 with the message.
int write_contributed(const cwc_ptau::View& view, const uint8_t* const bodies[5], const Section7& s, void** out, size_t* out_len, gw_status_t* status);

inline int fail2(gw_status_t* status, const std::string& msg) {  // a failure that is not a verdict about the file
    cwc_r1cs::set_status(status, msg);
    return 2;
}

}  // namespace cwc_ceremony
