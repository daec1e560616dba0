// Section 10 of a `.zkey`, read and written; BLAKE2b-512; the transcript of a phase-2 contribution and its challenge point
// (include/graph_witness_groth16_contribute.h has the definitions).  Host only: the few points of a record are handled by
// the host build of fq_gfx950.hpp.
//
//   64 B csHash | u32 nContributions | per record:
//     deltaAfter G1 64 B | g1_s G1 64 B | g1_sx G1 64 B | g2_spx G2 128 B | transcript 64 B
//     u32 type (0 = contribution, 1 = beacon) | u32 paramsLen | params
//   params: tagged items  01 len name[len]  |  02 numIterationsExp  |  03 len beaconHash[len]
#include <string.h>

#include <stdlib.h>

#include "beacon.hpp"
#include "binfile.hpp"
#include "contribute_internal.hpp"
#include "g2_subgroup_gfx950.hpp"
#include "../../include/graph_witness_groth16_beacon.h"
#include "../../include/graph_witness_groth16_contribute.h"

using namespace cwc_g16;
using cwc::Fr;
using cwc_r1cs::rd32;

namespace cwc_contrib {

// ---- BLAKE2b ----------------------------------------------------------------------------------------------------------------
namespace {

const uint64_t IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                        0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
const uint8_t SIGMA[12][16] = {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
                               {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
                               {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
                               {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
                               {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
                               {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};

inline uint64_t rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

}  // namespace

Blake2b::Blake2b() {
    memcpy(h_, IV, sizeof h_);
    h_[0] ^= 0x01010040ull;  // digest length 64, no key, fanout 1, depth 1
}

void Blake2b::compress(const uint8_t* block, bool last) {
    uint64_t m[16], v[16];
    memcpy(m, block, 128);  // little-endian words on a little-endian host
    memcpy(v, h_, sizeof h_);
    memcpy(v + 8, IV, sizeof IV);
    v[12] ^= t_;  // (the counter's high word stays 0: inputs here are far below 2^64 bytes)
    if (last) v[14] = ~v[14];
    auto G = [&](int a, int b, int c, int d, uint64_t x, uint64_t y) {
        v[a] = v[a] + v[b] + x;
        v[d] = rotr(v[d] ^ v[a], 32);
        v[c] = v[c] + v[d];
        v[b] = rotr(v[b] ^ v[c], 24);
        v[a] = v[a] + v[b] + y;
        v[d] = rotr(v[d] ^ v[a], 16);
        v[c] = v[c] + v[d];
        v[b] = rotr(v[b] ^ v[c], 63);
    };
    for (int r = 0; r < 12; ++r) {
        const uint8_t* s = SIGMA[r];
        G(0, 4, 8, 12, m[s[0]], m[s[1]]);
        G(1, 5, 9, 13, m[s[2]], m[s[3]]);
        G(2, 6, 10, 14, m[s[4]], m[s[5]]);
        G(3, 7, 11, 15, m[s[6]], m[s[7]]);
        G(0, 5, 10, 15, m[s[8]], m[s[9]]);
        G(1, 6, 11, 12, m[s[10]], m[s[11]]);
        G(2, 7, 8, 13, m[s[12]], m[s[13]]);
        G(3, 4, 9, 14, m[s[14]], m[s[15]]);
    }
    for (int i = 0; i < 8; ++i) h_[i] ^= v[i] ^ v[i + 8];
}

void Blake2b::update(const void* data, size_t len) {
    const uint8_t* p = (const uint8_t*)data;
    while (len) {
        if (fill_ == 128) {  // more input follows: the buffered block is not the last one
            t_ += 128;
            compress(buf_, false);
            fill_ = 0;
        }
        const size_t take = len < 128 - fill_ ? len : 128 - fill_;
        memcpy(buf_ + fill_, p, take);
        fill_ += take;
        p += take;
        len -= take;
    }
}

void Blake2b::final(uint8_t out[HASH_BYTES]) {
    t_ += fill_;
    memset(buf_ + fill_, 0, 128 - fill_);
    compress(buf_, true);
    memcpy(out, h_, HASH_BYTES);
}

void blake2b512(const void* data, size_t len, uint8_t out[HASH_BYTES]) {
    Blake2b b;
    b.update(data, len);
    b.final(out);
}

// ---- section 10 -------------------------------------------------------------------------------------------------------------
bool Section10::blank() const {
    if (!recs.empty()) return false;
    for (uint8_t b : cs_hash)
        if (b) return false;
    return true;
}

bool parse_section10(const uint8_t* p, uint64_t size, Section10& out, std::string& err) {
    const std::string pre = "zkey: section 10 ";
    if (size < HASH_BYTES + 4) {
        err = pre + "is truncated (" + std::to_string(size) + " bytes, 68 at the least)";
        return false;
    }
    memcpy(out.cs_hash, p, HASH_BYTES);
    const uint32_t n = rd32(p + HASH_BYTES);
    uint64_t off = HASH_BYTES + 4;
    if ((size - off) / RECORD_FIXED_BYTES < n) {
        err = pre + "declares " + std::to_string(n) + " contributions, which its " + std::to_string(size) + " bytes cannot hold";
        return false;
    }
    out.recs.clear();
    out.recs.resize(n);
    for (uint32_t k = 0; k < n; ++k) {
        const std::string who = pre + "contribution " + std::to_string(k + 1) + ": ";
        if (size - off < RECORD_FIXED_BYTES) {
            err = who + "the record is truncated";
            return false;
        }
        Record& r = out.recs[k];
        const uint8_t* q = p + off;
        memcpy(r.delta_after, q, G1_BYTES);
        memcpy(r.g1_s, q + 64, G1_BYTES);
        memcpy(r.g1_sx, q + 128, G1_BYTES);
        memcpy(r.g2_spx, q + 192, G2_BYTES);
        memcpy(r.transcript, q + 320, HASH_BYTES);
        const struct {
            const char* name;
            const uint8_t* at;
            bool g2;
        } pts[4] = {{"deltaAfter", r.delta_after, false}, {"g1_s", r.g1_s, false}, {"g1_sx", r.g1_sx, false}, {"g2_spx", r.g2_spx, true}};
        for (const auto& pt : pts) {
            const PointFault f = pt.g2 ? point_fault<G2>(pt.at, false) : point_fault<G1>(pt.at, false);
            if (f == PointFault::COORDINATE) {
                err = who + pt.name + " has a coordinate >= q";
                return false;
            }
            if (f == PointFault::CURVE) {
                err = who + pt.name + " is not on the " + (pt.g2 ? "G2" : "G1") + " curve";
                return false;
            }
        }
        r.type = rd32(q + PUB_BYTES);
        if (r.type > 1) {
            err = who + "unknown type " + std::to_string(r.type) + " (0 = contribution, 1 = beacon)";
            return false;
        }
        const uint32_t plen = rd32(q + PUB_BYTES + 4);
        off += RECORD_FIXED_BYTES;
        if (plen > size - off) {
            err = who + "paramsLen " + std::to_string(plen) + " runs past the section's end (" + std::to_string(size - off) + " bytes left)";
            return false;
        }
        const uint8_t* par = p + off;
        r.params.assign(par, par + plen);
        for (uint32_t i = 0; i < plen;) {
            const uint8_t tag = par[i++];
            if (tag == 2) {
                if (i >= plen) {
                    err = who + "parameter 02 (numIterationsExp) runs past the parameters' end";
                    return false;
                }
                ++i;
            } else if (tag == 1 || tag == 3) {
                if (i >= plen || (uint32_t)par[i] > plen - i - 1) {
                    err = who + "the length of parameter 0" + std::to_string(tag) + " runs past the parameters' end";
                    return false;
                }
                if (tag == 1) r.name.assign((const char*)par + i + 1, par[i]);
                i += 1u + par[i];
            } else {
                err = who + "unknown parameter tag " + std::to_string(tag);
                return false;
            }
        }
        off += plen;
    }
    if (off != size) {
        err = pre + "has " + std::to_string(size - off) + " trailing bytes after its last contribution";
        return false;
    }
    return true;
}

void write_section10(const Section10& s, std::vector<uint8_t>& out) {
    auto put32 = [&](uint32_t x) { out.insert(out.end(), (const uint8_t*)&x, (const uint8_t*)&x + 4); };
    out.insert(out.end(), s.cs_hash, s.cs_hash + HASH_BYTES);
    put32((uint32_t)s.recs.size());
    for (const Record& r : s.recs) {
        out.insert(out.end(), r.delta_after, r.delta_after + G1_BYTES);
        out.insert(out.end(), r.g1_s, r.g1_s + G1_BYTES);
        out.insert(out.end(), r.g1_sx, r.g1_sx + G1_BYTES);
        out.insert(out.end(), r.g2_spx, r.g2_spx + G2_BYTES);
        out.insert(out.end(), r.transcript, r.transcript + HASH_BYTES);
        put32(r.type);
        put32((uint32_t)r.params.size());
        out.insert(out.end(), r.params.begin(), r.params.end());
    }
}

std::vector<uint8_t> name_params(const std::string& name) {
    std::vector<uint8_t> v;
    if (!name.empty()) {
        v.push_back(1);
        v.push_back((uint8_t)name.size());
        v.insert(v.end(), name.begin(), name.end());
    }
    return v;
}

// ---- encodings --------------------------------------------------------------------------------------------------------------
namespace {

void be32(const Fq& mont, uint8_t* out) {  // canonical, big-endian
    const Fq c = fq_from_mont(mont);
    for (int i = 0; i < 32; ++i) out[i] = (uint8_t)(c.v[7 - i / 4] >> (8 * (3 - i % 4)));
}
void le32(const Fq& mont, uint8_t* out) {
    const Fq c = fq_from_mont(mont);
    memcpy(out, c.v, 32);
}

}  // namespace

void u1_bytes(const uint8_t* stored, uint8_t* out) {
    be32(rd_fq(stored), out);
    be32(rd_fq(stored + 32), out + 32);
}
void u2_bytes(const uint8_t* stored, uint8_t* out) {  // x.c1, x.c0, y.c1, y.c0
    be32(rd_fq(stored + 32), out);
    be32(rd_fq(stored), out + 32);
    be32(rd_fq(stored + 96), out + 64);
    be32(rd_fq(stored + 64), out + 96);
}
void canonical_g1(const uint8_t* stored, uint8_t* out) {
    for (int k = 0; k < 2; ++k) le32(rd_fq(stored + 32 * k), out + 32 * k);
}
void canonical_g2(const uint8_t* stored, uint8_t* out) {
    for (int k = 0; k < 4; ++k) le32(rd_fq(stored + 32 * k), out + 32 * k);
}

void pub_bytes(const Record& r, uint8_t out[PUB_BYTES]) {
    u1_bytes(r.delta_after, out);
    u1_bytes(r.g1_s, out + 64);
    u1_bytes(r.g1_sx, out + 128);
    u2_bytes(r.g2_spx, out + 192);
    memcpy(out + 320, r.transcript, HASH_BYTES);
}

void record_hash(const Record& r, uint8_t out[HASH_BYTES]) {
    uint8_t pub[PUB_BYTES];
    pub_bytes(r, pub);
    blake2b512(pub, sizeof pub, out);
}

void transcript_of(const Section10& s, size_t k, const uint8_t* g1_s, const uint8_t* g1_sx, uint8_t out[HASH_BYTES]) {
    Blake2b h;
    h.update(s.cs_hash, HASH_BYTES);
    uint8_t pub[PUB_BYTES];
    for (size_t i = 0; i < k; ++i) {
        pub_bytes(s.recs[i], pub);
        h.update(pub, sizeof pub);
    }
    u1_bytes(g1_s, pub);
    u1_bytes(g1_sx, pub + 64);
    h.update(pub, 128);
    h.final(out);
}

// ---- the challenge point ----------------------------------------------------------------------------------------------------
namespace {

Fq fq_pow(const Fq& a, const Fq& e) {  // Montgomery a, plain exponent
    Fq acc = fq_one();
    for (int b = 255; b >= 0; --b) {
        acc = fq_sqr(acc);
        if ((e.v[b >> 5] >> (b & 31)) & 1u) acc = fq_mul(acc, a);
    }
    return acc;
}

// a square root of a in Fq (q = 3 mod 4: a^((q + 1) / 4)), false when a is not a square
bool fq_sqrt(const Fq& a, Fq& root) {
    Fq e;
    cwc::u256_add(e, fq_p(), Fq{{1, 0, 0, 0, 0, 0, 0, 0}});
    root = fq_pow(a, cwc::u256_shr(e, 2));
    return cwc::u256_eq(fq_sqr(root), a);
}

// a square root of a in Fq2 by the norm method, false when a is not a square: with n = a0^2 + a1^2 = s^2, the root x0 + x1 u
// has x0^2 = (a0 + s) / 2 or (a0 - s) / 2 and x1 = a1 / (2 x0); a root with x0 = 0 is u sqrt(-a0)
bool fq2_sqrt(const Fq2& a, Fq2& root) {
    if (Fq2T::is_zero(a)) {
        root = a;
        return true;
    }
    Fq s;
    if (!fq_sqrt(fq_add(fq_sqr(a.c0), fq_sqr(a.c1)), s)) return false;
    const Fq half = fq_inv(fq_add(fq_one(), fq_one()));
    for (int k = 0; k < 2; ++k) {
        const Fq t = fq_mul(k == 0 ? fq_add(a.c0, s) : fq_sub(a.c0, s), half);
        Fq x0;
        if (!fq_sqrt(t, x0) || cwc::u256_is_zero(x0)) continue;
        root = Fq2{x0, fq_mul(a.c1, fq_inv(fq_dbl(x0)))};
        if (Fq2T::eq(fq2_sqr(root), a)) return true;
    }
    Fq x1;
    if (cwc::u256_is_zero(a.c1) && fq_sqrt(fq_neg(a.c0), x1)) {
        root = Fq2{fq_zero(), x1};
        return true;
    }
    return false;
}

// canonical (c1, c0) of a below that of b?
bool pair_less(const Fq2& a, const Fq2& b) {
    const Fq a1 = fq_from_mont(a.c1), b1 = fq_from_mont(b.c1);
    if (!cwc::u256_eq(a1, b1)) return cwc::u256_lt(a1, b1);
    return cwc::u256_lt(fq_from_mont(a.c0), fq_from_mont(b.c0));
}

}  // namespace

A2 hash_to_g2(const uint8_t t[HASH_BYTES]) {
    Fr cofactor, two_q;  // 2q - r, the order of E'(Fq2) over r
    cwc::u256_add(two_q, fq_p(), fq_p());
    cwc::u256_sub(cofactor, two_q, cwc::fr_p());
    for (uint32_t ctr = 0;; ++ctr) {
        uint8_t msg[HASH_BYTES + 6 + 4], d[HASH_BYTES];
        memcpy(msg, t, HASH_BYTES);
        memcpy(msg + HASH_BYTES, "cwc-g2", 6);
        memcpy(msg + HASH_BYTES + 6, &ctr, 4);
        blake2b512(msg, sizeof msg, d);
        Fq c0, c1;
        memcpy(c0.v, d, 32);
        memcpy(c1.v, d + 32, 32);
        c0.v[7] &= 0x3fffffffu;
        c1.v[7] &= 0x3fffffffu;
        if (!cwc::u256_lt(c0, fq_p()) || !cwc::u256_lt(c1, fq_p())) continue;
        const Fq2 x{fq_to_mont(c0), fq_to_mont(c1)};
        Fq2 y;
        if (!fq2_sqrt(fq2_add(fq2_mul(fq2_sqr(x), x), curve_b<G2>()), y)) continue;
        const Fq2 ny = fq2_neg(y);
        if (pair_less(ny, y)) y = ny;
        const P2 p = xyzz_mul(P2{x, y, Fq2T::one(), Fq2T::one()}, cofactor);
        if (xyzz_is_inf(p)) continue;
        return xyzz_to_affine(p);
    }
}

// ---- single points on the host ----------------------------------------------------------------------------------------------
void put_stored(uint8_t* out, const A1& p) { put_coords<G1>(out, p.x, p.y, false); }
void put_stored(uint8_t* out, const A2& p) { put_coords<G2>(out, p.x, p.y, false); }

void g1_mul_stored(const uint8_t* in, const Fr& k, uint8_t* out) {
    A1 a;
    get_coords<G1>(in, false, a.x, a.y);
    put_stored(out, xyzz_to_affine(xyzz_mul(from_affine(a), k)));
}
void g2_mul_stored(const uint8_t* in, const Fr& k, uint8_t* out) {
    A2 a;
    get_coords<G2>(in, false, a.x, a.y);
    put_stored(out, xyzz_to_affine(xyzz_mul(from_affine(a), k)));
}
bool g2_stored_in_subgroup(const uint8_t* in) {
    A2 a;
    get_coords<G2>(in, false, a.x, a.y);
    return g2_in_subgroup(a);
}

}  // namespace cwc_contrib

// ---- C ABI (host only) ------------------------------------------------------------------------------------------------------
using namespace cwc_contrib;

extern "C" {

void gwb_blake2b512(const void* data, size_t len, void* out64) { blake2b512(data, len, (uint8_t*)out64); }

void gwb_sha256(const void* data, size_t len, void* out32) { cwc_beacon::sha256(data, len, (uint8_t*)out32); }

int gwb_beacon_scalars(uint32_t phase, const void* beacon_hash, size_t hash_len, uint32_t iterations_exp, void* out) {
    if (!out || !beacon_hash || (phase != 1 && phase != 2)) return 2;
    if (!cwc_beacon::argument_fault(0, hash_len, iterations_exp, cwc_beacon::limit()).empty()) return 2;
    Fr x[cwc_beacon::PHASE1_SCALARS];
    cwc_beacon::scalars(phase, (const uint8_t*)beacon_hash, hash_len, iterations_exp, x);
    for (uint32_t j = 0; j < cwc_beacon::scalar_count(phase); ++j) memcpy((uint8_t*)out + 32 * j, x[j].v, 32);
    return 0;
}

int gwb_zkey_contribution_params(const void* zkey, size_t len, size_t k, void** out, size_t* out_len, gw_status_t* status) {
    auto fail2 = [&](const std::string& msg) {
        cwc_r1cs::set_status(status, msg);
        return 2;
    };
    if (!out || !out_len || (!zkey && len)) return fail2("gwb_zkey_contribution_params: NULL argument");
    *out = nullptr;
    *out_len = 0;
    try {
        cwc_r1cs::BinSection secs[11];
        std::string err;
        if (!cwc_r1cs::binfile_sections((const uint8_t*)zkey, len, "zkey", 0x7feu, secs, err)) return fail2(err);
        if (!secs[10].p) return fail2("zkey: section 10 is missing");
        Section10 s;
        if (!parse_section10(secs[10].p, secs[10].size, s, err)) return fail2(err);
        if (k >= s.recs.size()) return fail2("zkey: there is no contribution " + std::to_string(k + 1) + " (the key has " + std::to_string(s.recs.size()) + ")");
        const std::vector<uint8_t>& par = s.recs[k].params;
        void* buf = malloc(par.size() ? par.size() : 1);
        if (!buf) return fail2("zkey: out of host memory");
        if (!par.empty()) memcpy(buf, par.data(), par.size());
        *out = buf;
        *out_len = par.size();
    } catch (const std::bad_alloc&) {
        return fail2("zkey: out of host memory");
    }
    cwc_r1cs::set_ok(status);
    return 0;
}

void gwb_zkey_contribution_challenge(const void* t64, void* out128) {
    uint8_t stored[G2_BYTES];
    put_stored(stored, hash_to_g2((const uint8_t*)t64));
    canonical_g2(stored, (uint8_t*)out128);
}

int gwb_zkey_contributions(const void* zkey, size_t len, void** out, size_t* out_len, gw_status_t* status) {
    if (!out || !out_len || (!zkey && len)) return cwc_r1cs::fail(status, "gwb_zkey_contributions: NULL argument");
    *out = nullptr;
    *out_len = 0;
    try {
        cwc_r1cs::BinSection secs[11];
        std::string err;
        if (!cwc_r1cs::binfile_sections((const uint8_t*)zkey, len, "zkey", 0x7feu, secs, err)) return cwc_r1cs::fail(status, err);
        if (!secs[10].p) return cwc_r1cs::fail(status, "zkey: section 10 is missing");
        Section10 s;
        if (!parse_section10(secs[10].p, secs[10].size, s, err)) return cwc_r1cs::fail(status, err);
        std::vector<uint8_t> v(s.cs_hash, s.cs_hash + HASH_BYTES);
        auto put32 = [&](uint32_t x) { v.insert(v.end(), (const uint8_t*)&x, (const uint8_t*)&x + 4); };
        put32((uint32_t)s.recs.size());
        for (const Record& r : s.recs) {
            uint8_t b[3 * G1_BYTES + G2_BYTES + 2 * HASH_BYTES];
            canonical_g1(r.delta_after, b);
            canonical_g1(r.g1_s, b + 64);
            canonical_g1(r.g1_sx, b + 128);
            canonical_g2(r.g2_spx, b + 192);
            memcpy(b + 320, r.transcript, HASH_BYTES);
            record_hash(r, b + 384);
            v.insert(v.end(), b, b + sizeof b);
            put32(r.type);
            put32((uint32_t)r.name.size());
            v.insert(v.end(), r.name.begin(), r.name.end());
        }
        void* buf = malloc(v.size());
        if (!buf) return cwc_r1cs::fail(status, "zkey: out of host memory");
        memcpy(buf, v.data(), v.size());
        *out = buf;
        *out_len = v.size();
    } catch (const std::bad_alloc&) {
        return cwc_r1cs::fail(status, "zkey: out of host memory");
    }
    cwc_r1cs::set_ok(status);
    return 0;
}

}  // extern "C"
