// `.r1cs` loader (iden3 binfile "r1cs" version 1, as circom writes it): hostile bytes in, a validated gwb_r1cs or a
// message out.  All integers little-endian; sections in any order.
//   file:      "r1cs", u32 version = 1, u32 nSections, then per section u32 type, u64 size, size bytes
//   section 1: u32 n8, prime (n8 bytes), u32 nWires, nPubOut, nPubIn, nPrvIn, u64 nLabels, u32 nConstraints
//   section 2: nConstraints x (A, B, C), each combination u32 nFactors + nFactors x (u32 wire, n8-byte coefficient)
//   section 3: nWires x u64 label id
//   sections 4, 5: custom gates (refused)
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <unordered_map>

#include "r1cs_internal.hpp"

using namespace cwc_r1cs;
using cwc::Fr;

namespace cwc_r1cs {

void set_status(gw_status_t* st, const std::string& msg) {
    if (!st) return;
    st->code = ERROR;
    st->error_msg = strdup(msg.c_str());
}
void set_ok(gw_status_t* st) {
    if (!st) return;
    st->code = OK;
    st->error_msg = nullptr;
}

}  // namespace cwc_r1cs

namespace {

struct Fail {
    std::string msg;
};

// bounded reader over [p, p + n)
struct Cur {
    const uint8_t* p;
    uint64_t n, off = 0;
    const char* what;
    uint64_t left() const { return n - off; }
    void need(uint64_t k) const {
        if (k > left()) throw Fail{std::string("r1cs: truncated ") + what};
    }
    uint32_t u32() {
        need(4);
        uint32_t v;
        memcpy(&v, p + off, 4);
        off += 4;
        return v;
    }
    uint64_t u64() {
        need(8);
        uint64_t v;
        memcpy(&v, p + off, 8);
        off += 8;
        return v;
    }
    Fr fr() {
        need(32);
        Fr v;
        memcpy(v.v, p + off, 32);
        off += 32;
        return v;
    }
};

bool fr_key_eq(const Fr& a, const Fr& b) { return memcmp(a.v, b.v, 32) == 0; }

struct FrHash {
    size_t operator()(const Fr& a) const {
        uint64_t h = 1469598103934665603ull;
        for (int i = 0; i < 8; ++i) h = (h ^ a.v[i]) * 1099511628211ull;
        return (size_t)h;
    }
};
struct FrEq {
    bool operator()(const Fr& a, const Fr& b) const { return fr_key_eq(a, b); }
};

struct Lc {
    std::vector<uint32_t> fac, cidx;
};

void load(const uint8_t* d, size_t len, gwb_r1cs& r) {
    Cur f{d, len, 0, "file header"};
    f.need(4);
    if (memcmp(d, "r1cs", 4) != 0) throw Fail{"r1cs: bad magic (not an .r1cs file)"};
    f.off = 4;
    const uint32_t version = f.u32();
    if (version != 1) throw Fail{"r1cs: unsupported version " + std::to_string(version) + " (1 expected)"};
    const uint32_t n_sections = f.u32();
    struct Sec {
        uint64_t off, size;
    };
    std::map<uint32_t, Sec> secs;
    for (uint32_t i = 0; i < n_sections; ++i) {
        f.what = "section header";
        const uint32_t type = f.u32();
        const uint64_t size = f.u64();
        if (size > f.left()) throw Fail{"r1cs: truncated section " + std::to_string(type) + " (declares " + std::to_string(size) +
                                        " bytes, " + std::to_string(f.left()) + " left)"};
        if (type == 4 || type == 5)
            throw Fail{"r1cs: custom gates are not supported (section " + std::to_string(type) +
                       (type == 4 ? ", custom gates list" : ", custom gates applications") + ")"};
        if (type >= 1 && type <= 3) {
            if (secs.count(type)) throw Fail{"r1cs: duplicate section " + std::to_string(type)};
            secs[type] = Sec{f.off, size};
        }
        f.off += size;
    }
    if (f.left() != 0) throw Fail{"r1cs: " + std::to_string(f.left()) + " trailing bytes after the last section"};
    static const char* names[4] = {"", "header", "constraints", "wire-to-label map"};
    for (uint32_t t = 1; t <= 3; ++t)
        if (!secs.count(t)) throw Fail{std::string("r1cs: missing section ") + std::to_string(t) + " (" + names[t] + ")"};

    // -- section 1
    Cur h{d + secs[1].off, secs[1].size, 0, "header section"};
    const uint32_t n8 = h.u32();
    if (n8 != 32) throw Fail{"r1cs: field size n8 = " + std::to_string(n8) + " (only BN254, n8 = 32, is supported)"};
    const Fr prime = h.fr();
    if (!fr_key_eq(prime, cwc::fr_p())) throw Fail{"r1cs: prime is not BN254's scalar field r (other fields are not supported)"};
    gwb_r1cs_info_t& in = r.info;
    RowSystem& sys = r.sys;
    in.n_wires = h.u32();
    in.n_pub_out = h.u32();
    in.n_pub_in = h.u32();
    in.n_prv_in = h.u32();
    in.n_labels = h.u64();
    in.n_constraints = h.u32();
    if (h.left() != 0) throw Fail{"r1cs: header section size " + std::to_string(secs[1].size) + " disagrees with its contents (64 bytes)"};
    if (in.n_wires == 0) throw Fail{"r1cs: nWires = 0 (wire 0 is the constant 1)"};
    if (in.n_wires > WIRE_MASK + 1ull) throw Fail{"r1cs: nWires = " + std::to_string(in.n_wires) + " is above 2^30"};
    if (1ull + in.n_pub_out + in.n_pub_in + in.n_prv_in > in.n_wires)
        throw Fail{"r1cs: 1 + nPubOut + nPubIn + nPrvIn exceeds nWires"};
    if (in.n_constraints > MAX_CONSTRAINTS) throw Fail{"r1cs: nConstraints = 0xFFFFFFFF is not supported"};

    // -- section 3
    {
        const uint64_t want = (uint64_t)in.n_wires * 8;  // u32 x 8: no overflow
        if (secs[3].size != want)
            throw Fail{"r1cs: wire-to-label map section size " + std::to_string(secs[3].size) + " disagrees with nWires x 8 = " + std::to_string(want)};
        r.wire_label.resize(in.n_wires);
        memcpy(r.wire_label.data(), d + secs[3].off, want);
        for (uint32_t i = 0; i < in.n_wires; ++i)
            if (r.wire_label[i] >= in.n_labels)
                throw Fail{"r1cs: wire " + std::to_string(i) + " maps to label " + std::to_string(r.wire_label[i]) + " >= nLabels"};
    }

    // -- section 2
    Cur c{d + secs[2].off, secs[2].size, 0, "constraints section"};
    // every constraint takes at least 12 bytes: refuse an impossible count before reserving for it
    if ((uint64_t)in.n_constraints * 12 > c.n)
        throw Fail{"r1cs: truncated constraints section (" + std::to_string(in.n_constraints) + " constraints cannot fit in " + std::to_string(c.n) + " bytes)"};
    const Fr one{{1, 0, 0, 0, 0, 0, 0, 0}};
    Fr minus_one = cwc::fr_p();
    minus_one.v[0] -= 1;
    std::unordered_map<Fr, uint32_t, FrHash, FrEq> coef_ix;
    std::vector<uint32_t> fac, cidx, rowptr;
    std::vector<uint32_t> len_of(in.n_constraints);
    rowptr.reserve(3ull * in.n_constraints + 1);
    rowptr.push_back(0);
    uint64_t nf_abc[3] = {0, 0, 0};
    for (uint32_t j = 0; j < in.n_constraints; ++j) {
        uint64_t total = 0;
        for (int k = 0; k < 3; ++k) {
            const uint32_t nf = c.u32();
            if ((uint64_t)nf * 36 > c.left())  // u32 x 36 fits u64
                throw Fail{"r1cs: truncated constraints section (constraint " + std::to_string(j) + " declares " + std::to_string(nf) + " factors)"};
            for (uint32_t q = 0; q < nf; ++q) {
                const uint32_t wire = c.u32();
                const Fr v = c.fr();
                if (wire >= in.n_wires)
                    throw Fail{"r1cs: constraint " + std::to_string(j) + " references wire " + std::to_string(wire) + " >= nWires = " + std::to_string(in.n_wires)};
                if (!cwc::u256_lt(v, cwc::fr_p()))
                    throw Fail{"r1cs: constraint " + std::to_string(j) + " has a coefficient >= r"};
                if (fr_key_eq(v, one)) {
                    fac.push_back(wire | (KIND_PLUS << 30));
                    cidx.push_back(0);
                } else if (fr_key_eq(v, minus_one)) {
                    fac.push_back(wire | (KIND_MINUS << 30));
                    cidx.push_back(0);
                } else {
                    auto it = coef_ix.find(v);
                    uint32_t ix;
                    if (it == coef_ix.end()) {
                        ix = (uint32_t)sys.coef.size();
                        coef_ix.emplace(v, ix);
                        sys.coef.push_back(cwc::fr_to_mont(v));
                    } else {
                        ix = it->second;
                    }
                    fac.push_back(wire | (KIND_GENERAL << 30));
                    cidx.push_back(ix);
                }
            }
            if (fac.size() > 0xffffffffull) throw Fail{"r1cs: more than 2^32 - 1 factors are not supported"};
            rowptr.push_back((uint32_t)fac.size());
            nf_abc[k] += nf;
            total += nf;
        }
        len_of[j] = (uint32_t)std::min<uint64_t>(total, 0xffffffffu);
    }
    if (c.left() != 0)
        throw Fail{"r1cs: constraints section size " + std::to_string(c.n) + " disagrees with its contents (" + std::to_string(c.off) + " bytes)"};
    in.n_factors_a = nf_abc[0];
    in.n_factors_b = nf_abc[1];
    in.n_factors_c = nf_abc[2];

    // Device order: constraints bucketed by the bit length of their factor count (a wave's lanes then walk constraints of
    // similar length), file order inside a bucket (neighbouring constraints tend to share wires).
    std::vector<uint32_t> order(in.n_constraints);
    for (uint32_t j = 0; j < in.n_constraints; ++j) order[j] = j;
    auto bucket = [&](uint32_t j) { return len_of[j] ? 32 - __builtin_clz(len_of[j]) : 0; };
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return bucket(a) < bucket(b); });
    sys.perm = order;
    sys.rowptr.reserve(rowptr.size());
    sys.fac.reserve(fac.size());
    sys.cidx.reserve(cidx.size());
    sys.rowptr.push_back(0);
    for (uint32_t j : order) {
        for (int k = 0; k < 3; ++k) {
            sys.fac.insert(sys.fac.end(), fac.begin() + rowptr[3ull * j + k], fac.begin() + rowptr[3ull * j + k + 1]);
            sys.cidx.insert(sys.cidx.end(), cidx.begin() + rowptr[3ull * j + k], cidx.begin() + rowptr[3ull * j + k + 1]);
            sys.rowptr.push_back((uint32_t)sys.fac.size());
        }
    }
    sys.n_rows = in.n_constraints;
    sys.n_wires = in.n_wires;
}

}  // namespace

extern "C" {

int gwb_r1cs_load(const void* data, size_t len, gwb_r1cs_t** out, gw_status_t* status) {
    if (!out || (!data && len)) {
        set_status(status, "gwb_r1cs_load: NULL argument");
        return 1;
    }
    gwb_r1cs* r = new (std::nothrow) gwb_r1cs();
    if (!r) {
        set_status(status, "gwb_r1cs_load: out of memory");
        return 1;
    }
    try {
        load((const uint8_t*)data, len, *r);
    } catch (const Fail& e) {
        delete r;
        set_status(status, e.msg);
        return 1;
    } catch (const std::bad_alloc&) {
        delete r;
        set_status(status, "r1cs: out of memory");
        return 1;
    }
    *out = r;
    set_ok(status);
    return 0;
}

int gwb_r1cs_info(const gwb_r1cs_t* r, gwb_r1cs_info_t* info) {
    if (!r || !info) return 1;
    *info = r->info;
    return 0;
}

int gwb_r1cs_set_tile_width(gwb_r1cs_t* r, uint32_t t) {
    if (!r || t > 64 || (t & (t - 1))) return 1;
    r->sys.tile_width = t;
    return 0;
}

}  // extern "C"
