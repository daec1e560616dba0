// The random beacon of both ceremony phases (include/graph_witness_groth16_beacon.h has the definitions): SHA-256, the hash
// chain, the derivation of a beacon's scalars, the beacon items of a record's parameters and the form rule of a type-1 record.
// Host only and header only: ceremony.cc, contributions.cc, ceremony.hip and contribute.hip include it, and the first two have to
// link without another object (tests/test_ptau_ceremony_host.py builds them on their own).  BLAKE2b is contributions.cc's.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../csrc/fr_gfx950.hpp"
#include "contribute_internal.hpp"

namespace cwc_beacon {

constexpr uint32_t MIN_EXP = 10, MAX_EXP = 63, DEFAULT_LIMIT = 28;  // snarkjs's range of numIterationsExp; the limit's default
constexpr size_t SHA256_BYTES = 32, HASH_MAX = 255;
constexpr uint32_t PHASE1_SCALARS = 6, PHASE2_SCALARS = 2;  // tau', alpha', beta', s_0, s_1, s_2  |  delta', s

// ---- SHA-256 (FIPS 180-4) ---------------------------------------------------------------------------------------------------
namespace detail {

inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

inline const uint32_t* sha256_k() {
    static const uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
        0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
        0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
        0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
        0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
        0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    return K;
}

inline void sha256_init(uint32_t h[8]) {
    static const uint32_t H0[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    memcpy(h, H0, sizeof H0);
}

// one block of sixteen big-endian words, already in host order in w[0 .. 16)
inline void sha256_compress(uint32_t h[8], uint32_t w[64]) {
    const uint32_t* K = sha256_k();
    for (int i = 16; i < 64; ++i) {
        const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
        const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
        w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], k = h[7];
    for (int i = 0; i < 64; ++i) {
        const uint32_t t1 = k + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        k = g;
        g = f;
        f = e;
        e = d + t1;
        d = c;
        c = b;
        b = a;
        a = t1 + t2;
    }
    h[0] += a;
    h[1] += b;
    h[2] += c;
    h[3] += d;
    h[4] += e;
    h[5] += f;
    h[6] += g;
    h[7] += k;
}

inline void sha256_block(uint32_t h[8], const uint8_t* block) {
    uint32_t w[64];
    for (int i = 0; i < 16; ++i)
        w[i] = ((uint32_t)block[4 * i] << 24) | ((uint32_t)block[4 * i + 1] << 16) | ((uint32_t)block[4 * i + 2] << 8) | (uint32_t)block[4 * i + 3];
    sha256_compress(h, w);
}

}  // namespace detail

inline void sha256(const void* data, size_t len, uint8_t out[SHA256_BYTES]) {
    const uint8_t* p = (const uint8_t*)data;
    uint32_t h[8];
    detail::sha256_init(h);
    size_t left = len;
    for (; left >= 64; left -= 64, p += 64) detail::sha256_block(h, p);
    uint8_t tail[128] = {};  // the last bytes, 0x80, zeros, the length in bits: one block, or two when fewer than 9 bytes are free
    if (left) memcpy(tail, p, left);
    tail[left] = 0x80;
    const size_t blocks = left + 9 <= 64 ? 1 : 2;
    const uint64_t bits = (uint64_t)len * 8;
    for (int i = 0; i < 8; ++i) tail[64 * blocks - 1 - i] = (uint8_t)(bits >> (8 * i));
    for (size_t b = 0; b < blocks; ++b) detail::sha256_block(h, tail + 64 * b);
    for (int i = 0; i < 8; ++i)
        for (int k = 0; k < 4; ++k) out[4 * i + k] = (uint8_t)(h[i] >> (8 * (3 - k)));
}

// D_0 = hash; D_{i+1} = SHA-256(D_i) for i < 2^exp; out = D_{2^exp}.  exp <= 63.  From D_1 on a link hashes 32 bytes, which is
// one block whose padding never changes: the digest's words go from one compression into the next without passing through bytes.
inline void chain(const uint8_t* hash, size_t hash_len, uint32_t exp, uint8_t out[SHA256_BYTES]) {
    uint8_t d[SHA256_BYTES];
    sha256(hash, hash_len, d);
    uint32_t h[8], w[64];
    for (int i = 0; i < 8; ++i) h[i] = ((uint32_t)d[4 * i] << 24) | ((uint32_t)d[4 * i + 1] << 16) | ((uint32_t)d[4 * i + 2] << 8) | (uint32_t)d[4 * i + 3];
    for (uint64_t left = (1ull << exp) - 1; left; --left) {
        memcpy(w, h, sizeof h);
        w[8] = 0x80000000u;
        for (int i = 9; i < 15; ++i) w[i] = 0;
        w[15] = 256;  // the length in bits
        detail::sha256_init(h);
        detail::sha256_compress(h, w);
    }
    for (int i = 0; i < 8; ++i)
        for (int k = 0; k < 4; ++k) out[4 * i + k] = (uint8_t)(h[i] >> (8 * (3 - k)));
}

// ---- the derivation ---------------------------------------------------------------------------------------------------------

// the big-endian integer of 64 bytes mod r, canonical: bit by bit, which no caller does often
inline cwc::Fr mod_r_be64(const uint8_t d[64]) {
    cwc::Fr acc = cwc::fr_zero();
    const cwc::Fr one{{1, 0, 0, 0, 0, 0, 0, 0}};
    for (int i = 0; i < 64; ++i)
        for (int b = 7; b >= 0; --b) {
            acc = cwc::fr_add(acc, acc);
            if ((d[i] >> b) & 1u) acc = cwc::fr_add(acc, one);
        }
    return acc;
}

// scalar(phase, j) from the chain's end D: the first nonzero value over ctr = 0, 1, ... of
// BLAKE2b-512("cwc-beacon" || u8(phase) || D || u8(j) || u32le(ctr)) mod r
inline cwc::Fr scalar_of(uint32_t phase, const uint8_t D[SHA256_BYTES], uint32_t j) {
    uint8_t msg[10 + 1 + SHA256_BYTES + 1 + 4], digest[cwc_contrib::HASH_BYTES];
    memcpy(msg, "cwc-beacon", 10);
    msg[10] = (uint8_t)phase;
    memcpy(msg + 11, D, SHA256_BYTES);
    msg[11 + SHA256_BYTES] = (uint8_t)j;
    for (uint32_t ctr = 0;; ++ctr) {
        memcpy(msg + 12 + SHA256_BYTES, &ctr, 4);  // little-endian host
        cwc_contrib::blake2b512(msg, sizeof msg, digest);
        const cwc::Fr x = mod_r_be64(digest);
        if (!cwc::u256_is_zero(x)) return x;
    }
}

inline uint32_t scalar_count(uint32_t phase) { return phase == 1 ? PHASE1_SCALARS : PHASE2_SCALARS; }

// The scalars of a beacon of phase 1 (six) or 2 (two), canonical, in the header's order.  The arguments are in range.
inline void scalars(uint32_t phase, const uint8_t* hash, size_t hash_len, uint32_t exp, cwc::Fr* out) {
    uint8_t D[SHA256_BYTES];
    chain(hash, hash_len, exp, D);
    for (uint32_t j = 0; j < scalar_count(phase); ++j) out[j] = scalar_of(phase, D, j);
}

// ---- the limit --------------------------------------------------------------------------------------------------------------

// CWC_BEACON_MAX_EXP when it is a decimal number in [10, 63], else 28; read once per process
inline uint32_t parse_limit(const char* v) {
    if (!v || !*v) return DEFAULT_LIMIT;
    char* end = nullptr;
    const unsigned long long x = strtoull(v, &end, 10);
    return *end == 0 && x >= MIN_EXP && x <= MAX_EXP ? (uint32_t)x : DEFAULT_LIMIT;
}
inline uint32_t limit() {
    static const uint32_t value = parse_limit(getenv("CWC_BEACON_MAX_EXP"));
    return value;
}
inline std::string over_limit(uint32_t exp, uint32_t lim) {
    return "numIterationsExp " + std::to_string(exp) + " is above the limit " + std::to_string(lim) + " (CWC_BEACON_MAX_EXP)";
}

// ---- a record's parameters --------------------------------------------------------------------------------------------------

// 01 name (omitted when empty) | 02 exp | 03 len hash: the order of a beacon made here.  name and hash of at most 255 bytes.
inline std::vector<uint8_t> write_params(const std::string& name, uint32_t exp, const uint8_t* hash, size_t hash_len) {
    std::vector<uint8_t> v = cwc_contrib::name_params(name);
    v.push_back(2);
    v.push_back((uint8_t)exp);
    v.push_back(3);
    v.push_back((uint8_t)hash_len);
    v.insert(v.end(), hash, hash + hash_len);
    return v;
}

// The beacon items of a record's tagged parameters: how many items 02 and 03 there are, and the last of each.
struct Items {
    uint32_t n_exp = 0, n_hash = 0, exp = 0;
    const uint8_t* hash = nullptr;  // into the parameters
    size_t hash_len = 0;
};
// Any bytes in; false when an item runs past the end or a tag is unknown (the section readers refuse those before).
inline bool read_params(const uint8_t* par, size_t plen, Items& out) {
    out = Items{};
    for (size_t i = 0; i < plen;) {
        const uint8_t tag = par[i++];
        if (tag == 2) {
            if (i >= plen) return false;
            out.exp = par[i++];
            ++out.n_exp;
        } else if (tag == 1 || tag == 3) {
            if (i >= plen || (size_t)par[i] > plen - i - 1) return false;
            if (tag == 3) {
                out.hash = par + i + 1;
                out.hash_len = par[i];
                ++out.n_hash;
            }
            i += 1u + par[i];
        } else {
            return false;
        }
    }
    return true;
}

// The rules about a type-1 record that need its parameters alone.  rc 0; 1 with the rule that fails (`msg` without the record's
// prefix); 2 when the record asks for more iterations than this process allows, which is no verdict about the file.
struct Form {
    int rc = 0;
    std::string msg;
    Items items;
};
inline Form form_of(const std::vector<uint8_t>& params, uint32_t lim) {
    Form f;
    if (!read_params(params.data(), params.size(), f.items) || f.items.n_exp != 1 || f.items.n_hash != 1 || f.items.hash_len == 0) {
        f.rc = 1;
        f.msg = f.items.n_exp > 1 || f.items.n_hash > 1 ? "a beacon record has more than one numIterationsExp or beaconHash"
                : f.items.n_hash == 1 && f.items.n_exp == 1 ? "a beacon record's beaconHash is empty"
                                                              : "a beacon record needs numIterationsExp and beaconHash";
        return f;
    }
    if (f.items.exp < MIN_EXP || f.items.exp > MAX_EXP) {
        f.rc = 1;
        f.msg = "numIterationsExp " + std::to_string(f.items.exp) + " is not in [" + std::to_string(MIN_EXP) + ", " + std::to_string(MAX_EXP) + "]";
    } else if (f.items.exp > lim) {
        f.rc = 2;
        f.msg = over_limit(f.items.exp, lim);
    }
    return f;
}

// form_of over the type-1 records among records [first, end) of a section (PtauRecord or Record), which a verification runs
// right after the file parses and before the device is touched: the first record that fails, as "<file>: contribution k: ...".
template <class Recs>
int forms_of(const Recs& recs, size_t first, const char* file, std::string& msg) {
    for (size_t k = first; k < recs.size(); ++k) {
        if (recs[k].type != 1) continue;
        const Form f = form_of(recs[k].params, limit());
        if (f.rc != 0) {
            msg = std::string(file) + ": contribution " + std::to_string(k + 1) + ": " + f.msg;
            return f.rc;
        }
    }
    return 0;
}

// What the making calls refuse about their own arguments, "" when they are fine; `rc` as above is always 2 for them.
inline std::string argument_fault(size_t name_len, size_t hash_len, uint32_t exp, uint32_t lim) {
    if (exp < MIN_EXP || exp > MAX_EXP) return "beacon: numIterationsExp " + std::to_string(exp) + " is not in [10, 63]";
    if (exp > lim) return "beacon: " + over_limit(exp, lim);
    if (hash_len == 0) return "beacon: the beaconHash is empty";
    if (hash_len > HASH_MAX) return "beacon: the beaconHash has " + std::to_string(hash_len) + " bytes, 255 at the most";
    if (name_len > 255) return "beacon: the name has " + std::to_string(name_len) + " bytes, 255 at the most";
    return "";
}

}  // namespace cwc_beacon
