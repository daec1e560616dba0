// Section 4 of a `.zkey` as the prover's witness map, and its comparison with an `.r1cs`.  Host code only: no device is touched.
//
// An entry (matrix m, constraint c, signal s, value v) stands for the term (v / R^2) w_s of a_c (m = 0) or b_c (m = 1), R = 2^256
// (snarkjs `zkey new` writes coefficients in doubled Montgomery form, and its buildABC1 multiplies them back out); c = a b for
// every row.  The public rows are ordinary entries (0, nC + i, i, R^2 mod r), i = 0..nPublic.  Entries come in any order, entries
// with the same (m, c, s) add up, a zero value contributes nothing, and a row without entries is zero.
//
// zkey_coefs_build turns the entries the loader kept (zkey.cc: matrix, constraint and signal already in range) into the arrays
// the evaluation kernel reads (a RowSystem, r1cs_internal.hpp): the factor stream wire | kind << 30 with KIND_PLUS / KIND_MINUS for v = +-R^2,
// the distinct other values as c R (one fr_from_mont of the file value), rows bucketed by length with perm back to the
// constraint index, and two row pointers per row.  Entries with the same (m, c, s) stay separate factors: the kernel's sum adds them.
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "groth16_internal.hpp"

using namespace cwc_r1cs;
using cwc::Fr;

namespace {

constexpr size_t ENTRY_BYTES = 44;
constexpr uint32_t MAX_POWER = 27;  // qap.hip: the coset needs a 2n-th root of unity and r has 2-adicity 28

struct Entry {
    uint32_t m, c, s;
    Fr v;
};

Entry entry_at(const gwb_zkey* z, uint64_t k) {
    const uint8_t* p = z->sec4.data() + k * ENTRY_BYTES;
    Entry e;
    memcpy(&e.m, p, 4);
    memcpy(&e.c, p + 4, 4);
    memcpy(&e.s, p + 8, 4);
    memcpy(e.v.v, p + 12, 32);
    return e;
}

uint64_t n_entries(const gwb_zkey* z) { return z->sec4.size() / ENTRY_BYTES; }

bool values_below_r(const gwb_zkey* z, std::string& err) {
    for (uint64_t k = 0, n = n_entries(z); k < n; ++k) {
        const Entry e = entry_at(z, k);
        if (!cwc::u256_lt(e.v, cwc::fr_p())) {
            err = "zkey: coefficient " + std::to_string(k) + " (matrix " + (e.m ? "B" : "A") + ", constraint " + std::to_string(e.c) + ", signal " +
                  std::to_string(e.s) + ") has a value >= r";
            return false;
        }
    }
    return true;
}

struct FrHash {
    size_t operator()(const Fr& a) const {
        uint64_t h = 1469598103934665603ull;
        for (int i = 0; i < 8; ++i) h = (h ^ a.v[i]) * 1099511628211ull;
        return (size_t)h;
    }
};
struct FrEq {
    bool operator()(const Fr& a, const Fr& b) const { return memcmp(a.v, b.v, 32) == 0; }
};

bool build(gwb_zkey* z, std::string& err) {
    const gwb_zkey_info_t& in = z->info;
    const uint64_t n = n_entries(z);
    if (n == 0) {
        err = "zkey: section 4 carries no coefficients (a key snarkjs writes has at least the row of wire 0), so the witness map cannot "
              "come from this key: pass the .r1cs instead";
        return false;
    }
    if (in.domain_size < 2 || in.domain_size > (1u << MAX_POWER)) {
        err = "zkey: domainSize " + std::to_string(in.domain_size) + " is outside 2 .. 2^27 (the witness map's coset needs a 2n-th root of unity and r has 2-adicity 28)";
        return false;
    }
    if (in.n_vars > WIRE_MASK + 1ull) {
        err = "zkey: nVars = " + std::to_string(in.n_vars) + " is above 2^30";
        return false;
    }
    if (!values_below_r(z, err)) return false;
    uint32_t max_c = 0;
    for (uint64_t k = 0; k < n; ++k) max_c = std::max(max_c, entry_at(z, k).c);
    const uint32_t n_used = max_c + 1;  // c < domainSize <= 2^27
    // factors per row and side (zero values are no factors)
    std::vector<uint32_t> len(2ull * n_used, 0);
    for (uint64_t k = 0; k < n; ++k) {
        const Entry e = entry_at(z, k);
        if (!cwc::u256_is_zero(e.v)) ++len[2ull * e.c + e.m];
    }
    // device order: rows bucketed by the bit length of their factor count, constraint order inside a bucket (loader.cc)
    std::vector<uint32_t> order(n_used);
    for (uint32_t c = 0; c < n_used; ++c) order[c] = c;
    auto bucket = [&](uint32_t c) {
        const uint64_t total = (uint64_t)len[2ull * c] + len[2ull * c + 1];  // <= n_coefs < 2^32
        return total ? 64 - __builtin_clzll(total) : 0;
    };
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return bucket(a) < bucket(b); });
    std::vector<uint32_t> rowptr(2ull * n_used + 1), cursor(2ull * n_used);
    uint32_t at = 0;
    for (uint32_t k = 0; k < n_used; ++k)
        for (uint32_t m = 0; m < 2; ++m) {
            rowptr[2ull * k + m] = at;
            cursor[2ull * order[k] + m] = at;
            at += len[2ull * order[k] + m];
        }
    rowptr[2ull * n_used] = at;
    std::vector<uint32_t> fac(at), cidx(at, 0);
    std::vector<Fr> coef;
    std::unordered_map<Fr, uint32_t, FrHash, FrEq> coef_ix;
    const Fr plus = cwc::fr_r2(), minus = cwc::fr_neg(plus);
    for (uint64_t k = 0; k < n; ++k) {
        const Entry e = entry_at(z, k);
        if (cwc::u256_is_zero(e.v)) continue;
        const uint32_t o = cursor[2ull * e.c + e.m]++;
        if (cwc::u256_eq(e.v, plus)) {
            fac[o] = e.s | (KIND_PLUS << 30);
        } else if (cwc::u256_eq(e.v, minus)) {
            fac[o] = e.s | (KIND_MINUS << 30);
        } else {
            auto it = coef_ix.find(e.v);
            uint32_t ix;
            if (it == coef_ix.end()) {
                ix = (uint32_t)coef.size();
                coef_ix.emplace(e.v, ix);
                coef.push_back(cwc::fr_from_mont(e.v));  // c R^2 -> c R
            } else {
                ix = it->second;
            }
            fac[o] = e.s | (KIND_GENERAL << 30);
            cidx[o] = ix;
        }
    }
    RowSystem& sys = z->sys;  // (stride 2 since the handle was made)
    sys.n_rows = n_used;
    sys.n_wires = in.n_vars;
    sys.rowptr.swap(rowptr);
    sys.fac.swap(fac);
    sys.cidx.swap(cidx);
    sys.perm.swap(order);
    sys.coef.swap(coef);
    z->coefs_built = true;
    return true;
}

// One side of the comparison: terms keyed by (constraint, matrix, signal), values in one common form
struct Term {
    uint64_t c;
    uint32_t m, s;
    Fr v;
};

bool key_lt(const Term& a, const Term& b) { return a.c != b.c ? a.c < b.c : a.m != b.m ? a.m < b.m : a.s < b.s; }
bool key_eq(const Term& a, const Term& b) { return a.c == b.c && a.m == b.m && a.s == b.s; }

// sorted by key, equal keys summed, zero sums dropped, every value through `canon`
template <class F>
void normalise(std::vector<Term>& t, F canon) {
    std::stable_sort(t.begin(), t.end(), key_lt);
    size_t out = 0;
    for (size_t i = 0; i < t.size();) {
        Term acc = t[i];
        size_t j = i + 1;
        for (; j < t.size() && key_eq(t[j], acc); ++j) acc.v = cwc::fr_add(acc.v, t[j].v);
        i = j;
        if (cwc::u256_is_zero(acc.v)) continue;
        acc.v = canon(acc.v);
        t[out++] = acc;
    }
    t.resize(out);
}

int refuse(gw_status_t* st, const std::string& msg) {
    set_status(st, msg);
    return 1;
}

int check_r1cs(const gwb_zkey* z, const gwb_r1cs* r, gw_status_t* status) {
    std::string err;
    if (!values_below_r(z, err)) return refuse(status, err);
    // section 4: values c R^2, summed in that form
    std::vector<Term> zt;
    zt.reserve(n_entries(z));
    for (uint64_t k = 0, n = n_entries(z); k < n; ++k) {
        const Entry e = entry_at(z, k);
        zt.push_back(Term{e.c, e.m, e.s, e.v});
    }
    normalise(zt, [](const Fr& v) { return cwc::fr_from_mont(cwc::fr_from_mont(v)); });
    // the .r1cs: A and B of every constraint at its file index (values c R), then the public rows
    const gwb_r1cs_info_t& ri = r->info;
    const RowSystem& rs = r->sys;
    const uint32_t nc = ri.n_constraints;
    const uint64_t n_pub = (uint64_t)ri.n_pub_out + ri.n_pub_in;
    std::vector<Term> rt;
    rt.reserve(ri.n_factors_a + ri.n_factors_b + n_pub + 1);
    const Fr one = cwc::fr_one(), minus_one = cwc::fr_neg(one);
    for (uint32_t k = 0; k < nc; ++k)
        for (uint32_t m = 0; m < 2; ++m)
            for (uint32_t j = rs.rowptr[3ull * k + m]; j < rs.rowptr[3ull * k + m + 1]; ++j) {
                const uint32_t f = rs.fac[j], kind = f >> 30;
                rt.push_back(Term{rs.perm[k], m, f & WIRE_MASK, kind == KIND_PLUS ? one : kind == KIND_MINUS ? minus_one : rs.coef[rs.cidx[j]]});
            }
    for (uint64_t s = 0; s <= n_pub; ++s) rt.push_back(Term{(uint64_t)nc + s, 0, (uint32_t)s, one});
    normalise(rt, [](const Fr& v) { return cwc::fr_from_mont(v); });
    // the smallest key at which the two differ
    const Term* at = nullptr;
    for (size_t i = 0; !at && (i < zt.size() || i < rt.size()); ++i) {
        if (i >= zt.size()) at = &rt[i];
        else if (i >= rt.size()) at = &zt[i];
        else if (!key_eq(zt[i], rt[i])) at = key_lt(zt[i], rt[i]) ? &zt[i] : &rt[i];
        else if (!cwc::u256_eq(zt[i].v, rt[i].v)) at = &zt[i];
    }
    if (at)
        return refuse(status, "zkey: section 4 differs from the r1cs at constraint " + std::to_string(at->c) + ", matrix " + (at->m ? "B" : "A") +
                                  ", signal " + std::to_string(at->s));
    // the same terms: the size fields
    const uint64_t n_rows = (uint64_t)nc + n_pub + 1;
    uint32_t p = 1;
    while ((1ull << p) < n_rows) ++p;
    const gwb_zkey_info_t& zi = z->info;
    if (zi.n_vars != ri.n_wires)
        return refuse(status, "zkey: section 4 holds the terms of the r1cs, but nVars " + std::to_string(zi.n_vars) + " != r1cs nWires " + std::to_string(ri.n_wires));
    if (zi.n_public != n_pub)
        return refuse(status, "zkey: section 4 holds the terms of the r1cs, but nPublic " + std::to_string(zi.n_public) + " != r1cs nPubOut + nPubIn " + std::to_string(n_pub));
    if (zi.domain_size != 1ull << p)
        return refuse(status, "zkey: section 4 holds the terms of the r1cs, but domainSize " + std::to_string(zi.domain_size) + " != r1cs QAP domain 2^" + std::to_string(p));
    set_ok(status);
    return 0;
}

}  // namespace

namespace cwc_r1cs {

bool zkey_coefs_build(gwb_zkey* z, std::string& err) {
    if (z->coefs_built) return true;
    try {
        return build(z, err);
    } catch (const std::bad_alloc&) {
        err = "zkey: out of host memory building the witness map of section 4";
        return false;
    }
}

}  // namespace cwc_r1cs

extern "C" {

int gwb_zkey_set_tile_width(gwb_zkey_t* z, uint32_t t) {
    if (!z || t > 64 || (t & (t - 1))) return 1;
    z->sys.tile_width = t;
    return 0;
}

int gwb_zkey_qap_info(gwb_zkey_t* z, gwb_r1cs_qap_info_t* info, gw_status_t* status) {
    if (!z || !info) return refuse(status, "gwb_zkey_qap_info: NULL argument");
    std::string err;
    if (!zkey_coefs_build(z, err)) return refuse(status, err);
    uint32_t p = 0;
    while ((1u << p) < z->info.domain_size) ++p;
    info->n_rows = z->sys.n_rows;
    info->domain_power = p;
    info->domain_size = z->info.domain_size;
    info->workspace_bytes_per_row = 2ull * 32 << p;
    set_ok(status);
    return 0;
}

int gwb_zkey_check_r1cs(const gwb_zkey_t* z, const gwb_r1cs_t* r, gw_status_t* status) {
    if (!z || !r) return refuse(status, "gwb_zkey_check_r1cs: NULL argument");
    try {
        return check_r1cs(z, r, status);
    } catch (const std::bad_alloc&) {
        return refuse(status, "zkey: out of host memory comparing section 4 with the r1cs");
    }
}

}  // extern "C"
