// The host side of a powers-of-tau ceremony (include/graph_witness_groth16_ceremony.h): a new `.ptau`, section 7 (hostile bytes
// in, a message that starts "ptau: section 7" out), the transcript, the image of a contributed file and the dump of the records.
// BLAKE2b, U1, U2, hash_to_g2 and the tagged parameters are contributions.cc's; the section table is binfile.hpp's.
#include <stdlib.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "../../include/graph_witness_groth16_beacon.h"
#include "../../include/graph_witness_groth16_ceremony.h"
#include "binfile.hpp"
#include "bn254_points_gfx950.hpp"
#include "ceremony_internal.hpp"
#include "contribute_internal.hpp"
#include "ptau_internal.hpp"

using namespace cwc_g16;
using namespace cwc_contrib;
using cwc_r1cs::rd32;

namespace cwc_ceremony {

namespace {

// the stored points of a record in record order: the five after-values, then the nine key points
struct RecordPoint {
    const char* name;
    size_t at;  // offset in the record
    bool g2;
};
const RecordPoint RECORD_POINTS[14] = {{"tauG1", 0, false},        {"tauG2", 64, true},         {"alphaG1", 192, false},      {"betaG1", 256, false},
                                       {"betaG2", 320, true},      {"tau_g1_s", 448, false},    {"tau_g1_sx", 512, false},    {"alpha_g1_s", 576, false},
                                       {"alpha_g1_sx", 640, false}, {"beta_g1_s", 704, false},   {"beta_g1_sx", 768, false},   {"tau_g2_spx", 832, true},
                                       {"alpha_g2_spx", 960, true}, {"beta_g2_spx", 1088, true}};

// the record's points as they lie in the file (PUB_BYTES)
void record_points(const PtauRecord& r, uint8_t* out) {
    memcpy(out, r.tau_g1, G1_BYTES);
    memcpy(out + 64, r.tau_g2, G2_BYTES);
    memcpy(out + 192, r.alpha_g1, G1_BYTES);
    memcpy(out + 256, r.beta_g1, G1_BYTES);
    memcpy(out + 320, r.beta_g2, G2_BYTES);
    for (int j = 0; j < 3; ++j) {
        memcpy(out + AFTER_BYTES + 2 * j * G1_BYTES, r.g1_s[j], G1_BYTES);
        memcpy(out + AFTER_BYTES + (2 * j + 1) * G1_BYTES, r.g1_sx[j], G1_BYTES);
        memcpy(out + AFTER_BYTES + 6 * G1_BYTES + j * G2_BYTES, r.g2_spx[j], G2_BYTES);
    }
}

void put32(std::vector<uint8_t>& v, uint32_t x) { v.insert(v.end(), (const uint8_t*)&x, (const uint8_t*)&x + 4); }

}  // namespace

bool parse_section7(const uint8_t* p, uint64_t size, Section7& out, std::string& err) {
    const std::string pre = "ptau: section 7 ";
    out.recs.clear();
    if (!p) return true;
    if (size < 4) {
        err = pre + "is truncated (" + std::to_string(size) + " bytes, 4 at the least)";
        return false;
    }
    const uint32_t n = rd32(p);
    uint64_t off = 4;
    if ((size - off) / RECORD_FIXED_BYTES < n) {
        err = pre + "declares " + std::to_string(n) + " contributions, which its " + std::to_string(size) + " bytes cannot hold";
        return false;
    }
    out.recs.resize(n);
    for (uint32_t k = 0; k < n; ++k) {
        const std::string who = pre + "contribution " + std::to_string(k + 1) + ": ";
        if (size - off < RECORD_FIXED_BYTES) {
            err = who + "the record is truncated";
            return false;
        }
        PtauRecord& r = out.recs[k];
        const uint8_t* q = p + off;
        for (const RecordPoint& pt : RECORD_POINTS) {
            const PointFault f = pt.g2 ? point_fault<G2>(q + pt.at, false) : point_fault<G1>(q + pt.at, false);
            if (f == PointFault::COORDINATE) {
                err = who + pt.name + " has a coordinate >= q";
                return false;
            }
            if (f == PointFault::CURVE) {
                err = who + pt.name + " is not on the " + (pt.g2 ? "G2" : "G1") + " curve";
                return false;
            }
        }
        memcpy(r.tau_g1, q, G1_BYTES);
        memcpy(r.tau_g2, q + 64, G2_BYTES);
        memcpy(r.alpha_g1, q + 192, G1_BYTES);
        memcpy(r.beta_g1, q + 256, G1_BYTES);
        memcpy(r.beta_g2, q + 320, G2_BYTES);
        for (int j = 0; j < 3; ++j) {
            memcpy(r.g1_s[j], q + AFTER_BYTES + 2 * j * G1_BYTES, G1_BYTES);
            memcpy(r.g1_sx[j], q + AFTER_BYTES + (2 * j + 1) * G1_BYTES, G1_BYTES);
            memcpy(r.g2_spx[j], q + AFTER_BYTES + 6 * G1_BYTES + j * G2_BYTES, G2_BYTES);
        }
        memcpy(r.partial_hash, q + PUB_BYTES, PARTIAL_HASH_BYTES);
        memcpy(r.next_challenge, q + PUB_BYTES + PARTIAL_HASH_BYTES, HASH_BYTES);
        const uint8_t* tail = q + PUB_BYTES + PARTIAL_HASH_BYTES + HASH_BYTES;
        r.type = rd32(tail);
        if (r.type > 1) {
            err = who + "unknown type " + std::to_string(r.type) + " (0 = contribution, 1 = beacon)";
            return false;
        }
        const uint32_t plen = rd32(tail + 4);
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

void write_section7(const Section7& s, std::vector<uint8_t>& out) {
    put32(out, (uint32_t)s.recs.size());
    uint8_t pts[PUB_BYTES];
    for (const PtauRecord& r : s.recs) {
        record_points(r, pts);
        out.insert(out.end(), pts, pts + PUB_BYTES);
        out.insert(out.end(), r.partial_hash, r.partial_hash + PARTIAL_HASH_BYTES);
        out.insert(out.end(), r.next_challenge, r.next_challenge + HASH_BYTES);
        put32(out, r.type);
        put32(out, (uint32_t)r.params.size());
        out.insert(out.end(), r.params.begin(), r.params.end());
    }
}

void pub_bytes(const PtauRecord& r, uint8_t out[PUB_BYTES]) {
    uint8_t pts[PUB_BYTES];
    record_points(r, pts);
    for (const RecordPoint& pt : RECORD_POINTS) {  // U1 and U2 are as long as the stored points
        if (pt.g2)
            u2_bytes(pts + pt.at, out + pt.at);
        else
            u1_bytes(pts + pt.at, out + pt.at);
    }
}

void next_challenge(const uint8_t challenge[HASH_BYTES], const PtauRecord& r, uint8_t out[HASH_BYTES]) {
    uint8_t pub[PUB_BYTES];
    pub_bytes(r, pub);
    Blake2b h;
    h.update(challenge, HASH_BYTES);
    h.update(pub, sizeof pub);
    h.final(out);
}

void last_challenge(const uint8_t* sec1, uint64_t sec1_size, const Section7& s, size_t k, uint8_t out[HASH_BYTES]) {
    if (k == 0)
        blake2b512(sec1, sec1_size, out);
    else
        memcpy(out, s.recs[k - 1].next_challenge, HASH_BYTES);
}

A2 key_challenge_point(const uint8_t challenge[HASH_BYTES], uint32_t j, const uint8_t* g1_s, const uint8_t* g1_sx) {
    uint8_t msg[HASH_BYTES + 1 + 2 * G1_BYTES], t[HASH_BYTES];
    memcpy(msg, challenge, HASH_BYTES);
    msg[HASH_BYTES] = (uint8_t)j;
    u1_bytes(g1_s, msg + HASH_BYTES + 1);
    u1_bytes(g1_sx, msg + HASH_BYTES + 1 + G1_BYTES);
    blake2b512(msg, sizeof msg, t);
    return hash_to_g2(t);
}

namespace {

// a file image under construction in one malloc'd buffer that the caller of the C ABI frees
struct Image {
    uint8_t* p = nullptr;
    size_t len = 0, at = 0;
    ~Image() { free(p); }
    bool alloc(size_t bytes) {
        p = (uint8_t*)malloc(bytes ? bytes : 1);
        len = bytes;
        return p != nullptr;
    }
    void put(const void* src, size_t n) {
        memcpy(p + at, src, n);
        at += n;
    }
    void put32(uint32_t x) { put(&x, 4); }
    void section(uint32_t id, uint64_t size) {
        put32(id);
        put(&size, 8);
    }
    void* release() {
        void* r = p;
        p = nullptr;
        return r;
    }
};

}  // namespace

int write_contributed(const cwc_ptau::View& view, const uint8_t* const bodies[5], const Section7& s, void** out, size_t* out_len, gw_status_t* status) {
    std::vector<uint8_t> sec7;
    write_section7(s, sec7);
    auto dropped = [](uint32_t id) { return id >= 12 && id <= 15; };
    size_t total = 12;
    uint32_t count = 0;
    for (const cwc_r1cs::BinEntry& e : view.order) {
        if (dropped(e.id)) continue;
        total += 12 + (e.id == 7 ? sec7.size() : (size_t)e.size);
        ++count;
    }
    if (!view.sec[7].p) {
        total += 12 + sec7.size();
        ++count;
    }
    Image img;
    if (!img.alloc(total)) return fail2(status, "ptau contribute: cannot allocate the " + std::to_string(total) + " bytes of the new file");
    img.put("ptau", 4);
    img.put32(1);
    img.put32(count);
    for (const cwc_r1cs::BinEntry& e : view.order) {
        if (dropped(e.id)) continue;
        if (e.id == 7) {
            img.section(7, sec7.size());
            img.put(sec7.data(), sec7.size());
        } else {
            img.section(e.id, e.size);
            img.put(e.id >= 2 && e.id <= 6 ? bodies[e.id - 2] : e.p, (size_t)e.size);
        }
    }
    if (!view.sec[7].p) {
        img.section(7, sec7.size());
        img.put(sec7.data(), sec7.size());
    }
    *out_len = img.len;
    *out = img.release();
    cwc_r1cs::set_ok(status);
    return 0;
}

namespace {

int ptau_new(uint32_t power, void** out, size_t* out_len, gw_status_t* status) {
    if (power < 1 || power > cwc_ptau::MAX_POWER)
        return fail2(status, "ptau new: power " + std::to_string(power) + " is not in [1, " + std::to_string(cwc_ptau::MAX_POWER) + "]");
    const uint64_t np = 1ull << power;
    const uint64_t counts[5] = {2 * np - 1, np, np, np, 1};
    const bool g2[5] = {false, true, false, false, true};
    uint64_t total = 12 + (12 + 44) + (12 + 4);
    for (int i = 0; i < 5; ++i) total += 12 + counts[i] * (g2[i] ? G2_BYTES : G1_BYTES);
    Image img;
    if (total > SIZE_MAX || !img.alloc((size_t)total)) return fail2(status, "ptau new: cannot allocate the " + std::to_string(total) + " bytes of the file");
    uint8_t gen1[G1_BYTES], gen2[G2_BYTES];
    put_stored(gen1, g1_generator());
    put_stored(gen2, g2_generator());
    img.put("ptau", 4);
    img.put32(1);
    img.put32(7);
    img.section(1, 44);
    img.put32(32);
    const Fq q = fq_p();
    img.put(q.v, 32);
    img.put32(power);
    img.put32(power);
    for (int i = 0; i < 5; ++i) {
        const size_t pb = g2[i] ? G2_BYTES : G1_BYTES;
        img.section(2 + i, counts[i] * pb);
        for (uint64_t k = 0; k < counts[i]; ++k) img.put(g2[i] ? gen2 : gen1, pb);
    }
    img.section(7, 4);
    img.put32(0);
    *out_len = img.len;
    *out = img.release();
    cwc_r1cs::set_ok(status);
    return 0;
}

int contributions(const uint8_t* ptau, size_t len, void** out, size_t* out_len, gw_status_t* status) {
    std::string err;
    cwc_ptau::View view;
    Section7 s;
    if (!cwc_ptau::parse(ptau, len, view, err) || !parse_section7(view.sec[7].p, view.sec[7].size, s, err)) return fail2(status, err);
    std::vector<uint8_t> img;
    put32(img, (uint32_t)s.recs.size());
    uint8_t pts[PUB_BYTES], can[PUB_BYTES];
    for (const PtauRecord& r : s.recs) {
        record_points(r, pts);
        for (const RecordPoint& pt : RECORD_POINTS) {
            if (pt.g2)
                canonical_g2(pts + pt.at, can + pt.at);
            else
                canonical_g1(pts + pt.at, can + pt.at);
        }
        img.insert(img.end(), can, can + PUB_BYTES);
        img.insert(img.end(), r.next_challenge, r.next_challenge + HASH_BYTES);
        put32(img, r.type);
        put32(img, (uint32_t)r.name.size());
        img.insert(img.end(), r.name.begin(), r.name.end());
    }
    void* buf = malloc(img.size());
    if (!buf) return fail2(status, "ptau: out of host memory");
    memcpy(buf, img.data(), img.size());
    *out = buf;
    *out_len = img.size();
    cwc_r1cs::set_ok(status);
    return 0;
}

}  // namespace

}  // namespace cwc_ceremony

extern "C" {

int gwb_ptau_new(uint32_t power, void** out, size_t* out_len, gw_status_t* status) {
    if (!out || !out_len) return cwc_ceremony::fail2(status, "gwb_ptau_new: NULL argument");
    *out = nullptr;
    *out_len = 0;
    return cwc_ceremony::ptau_new(power, out, out_len, status);
}

int gwb_ptau_contributions(const void* ptau, size_t len, void** out, size_t* out_len, gw_status_t* status) {
    if (!out || !out_len || (!ptau && len)) return cwc_ceremony::fail2(status, "gwb_ptau_contributions: NULL argument");
    *out = nullptr;
    *out_len = 0;
    try {
        return cwc_ceremony::contributions((const uint8_t*)ptau, len, out, out_len, status);
    } catch (const std::bad_alloc&) {
        return cwc_ceremony::fail2(status, "ptau: out of host memory");
    }
}

int gwb_ptau_contribution_params(const void* ptau, size_t len, size_t k, void** out, size_t* out_len, gw_status_t* status) {
    using cwc_ceremony::fail2;
    if (!out || !out_len || (!ptau && len)) return fail2(status, "gwb_ptau_contribution_params: NULL argument");
    *out = nullptr;
    *out_len = 0;
    try {
        std::string err;
        cwc_ptau::View view;
        cwc_ceremony::Section7 s;
        if (!cwc_ptau::parse((const uint8_t*)ptau, len, view, err) || !cwc_ceremony::parse_section7(view.sec[7].p, view.sec[7].size, s, err))
            return fail2(status, err);
        if (k >= s.recs.size())
            return fail2(status, "ptau: there is no contribution " + std::to_string(k + 1) + " (the file has " + std::to_string(s.recs.size()) + ")");
        const std::vector<uint8_t>& par = s.recs[k].params;
        void* buf = malloc(par.size() ? par.size() : 1);
        if (!buf) return fail2(status, "ptau: out of host memory");
        if (!par.empty()) memcpy(buf, par.data(), par.size());
        *out = buf;
        *out_len = par.size();
    } catch (const std::bad_alloc&) {
        return fail2(status, "ptau: out of host memory");
    }
    cwc_r1cs::set_ok(status);
    return 0;
}

}  // extern "C"
