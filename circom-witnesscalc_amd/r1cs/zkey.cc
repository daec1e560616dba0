// `.zkey` loader (iden3 binfile "zkey" version 1, Groth16, as snarkjs writes it): hostile bytes in, a validated gwb_zkey or a
// message out.  All integers little-endian; sections in any order.  Points are affine, uncompressed, every coordinate 32
// bytes in Montgomery form mod q (R = 2^256); a G2 point is x.c0, x.c1, y.c0, y.c1; all-zero bytes are the point at infinity.
//   file:       "zkey", u32 version = 1, u32 nSections, then per section u32 id, u64 size, size bytes
//   section 1:  u32 protocol (1 = Groth16; 2 = PLONK and 10 = fflonk are refused)
//   section 2:  u32 n8q, q, u32 n8r, r, u32 nVars, u32 nPublic, u32 domainSize, alpha1, beta1, beta2, gamma2, delta1, delta2
//   section 3:  IC, nPublic + 1 G1        section 4: u32 nCoefs, nCoefs x (u32 matrix, u32 constraint, u32 signal, 32 B value)
//   section 5:  A, nVars G1               section 6: B1, nVars G1            section 7: B2, nVars G2
//   section 8:  C, nVars - nPublic - 1 G1 section 9: H, domainSize G1         section 10: contributions (ignored)
// Every coordinate must be below q and every point other than infinity on its curve (G1: y^2 = x^3 + 3, G2: y^2 = x^3 +
// 3 / (9 + u)).  G2 points are not checked for subgroup membership here; gwb_zkey_check_g2 (subgroup.hip) checks beta2, gamma2,
// delta2 and section 7 on the device when asked (Groth16(zkey, check_g2=True), groth16-prove --check-g2).  The curve check uses
// the host build of fq_gfx950.hpp.
#include <string.h>

#include <map>
#include <string>

#include "fq_gfx950.hpp"
#include "groth16_internal.hpp"

using namespace cwc_g16;

namespace {

struct Fail {
    std::string msg;
};

constexpr uint32_t SEC_HEADER_BYTES = 4 + 32 + 4 + 32 + 12 + 3 * G1_BYTES + 3 * G2_BYTES;  // 660

uint32_t rd32(const uint8_t* p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

Fq rd_fq(const uint8_t* p) {
    Fq v;
    memcpy(v.v, p, 32);
    return v;
}

Fq2 g2_b() {  // 3 / (9 + u), Montgomery form
    const Fq2 t{fq_to_mont(Fq{{9, 0, 0, 0, 0, 0, 0, 0}}), fq_one()};
    const Fq three = fq_to_mont(Fq{{3, 0, 0, 0, 0, 0, 0, 0}});
    const Fq2 i = fq2_inv(t);
    return Fq2{fq_mul(i.c0, three), fq_mul(i.c1, three)};
}

// n points of `words` coordinates each at p: coordinates below q, on the curve unless all zero
void check_points(const char* what, const uint8_t* p, uint64_t n, bool g2) {
    const Fq b1 = fq_to_mont(Fq{{3, 0, 0, 0, 0, 0, 0, 0}});
    static const Fq2 b2 = g2_b();
    const uint32_t words = g2 ? 4 : 2;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* pt = p + i * words * 32;
        bool zero = true;
        for (uint32_t k = 0; k < words; ++k) {
            const Fq c = rd_fq(pt + 32 * k);
            if (!cwc::u256_lt(c, fq_p()))
                throw Fail{std::string("zkey: ") + what + " point " + std::to_string(i) + " has a coordinate >= q"};
            zero = zero && cwc::u256_is_zero(c);
        }
        if (zero) continue;
        const bool ok = g2 ? on_curve<Fq2T>(Affine<Fq2T>{Fq2{rd_fq(pt), rd_fq(pt + 32)}, Fq2{rd_fq(pt + 64), rd_fq(pt + 96)}}, b2)
                           : on_curve<FqT>(Affine<FqT>{rd_fq(pt), rd_fq(pt + 32)}, b1);
        if (!ok) throw Fail{std::string("zkey: ") + what + " point " + std::to_string(i) + " is not on the " + (g2 ? "G2" : "G1") + " curve"};
    }
}

void load(const uint8_t* d, size_t len, gwb_zkey& z) {
    if (len < 12 || memcmp(d, "zkey", 4) != 0) throw Fail{"zkey: bad magic (not a .zkey file)"};
    const uint32_t version = rd32(d + 4), n_sections = rd32(d + 8);
    if (version != 1) throw Fail{"zkey: unsupported version " + std::to_string(version) + " (1 expected)"};
    struct Sec {
        uint64_t off, size;
    };
    std::map<uint32_t, Sec> secs;
    uint64_t off = 12;
    for (uint32_t i = 0; i < n_sections; ++i) {
        if (len - off < 12) throw Fail{"zkey: truncated section header"};
        const uint32_t id = rd32(d + off);
        uint64_t size;
        memcpy(&size, d + off + 4, 8);
        off += 12;
        if (size > len - off)
            throw Fail{"zkey: truncated section " + std::to_string(id) + " (declares " + std::to_string(size) + " bytes, " +
                       std::to_string(len - off) + " left)"};
        if (id >= 1 && id <= 10) {
            if (secs.count(id)) throw Fail{"zkey: duplicate section " + std::to_string(id)};
            secs[id] = Sec{off, size};
        }
        off += size;
    }
    if (off != len) throw Fail{"zkey: " + std::to_string(len - off) + " trailing bytes after the last section"};
    for (uint32_t id = 1; id <= 9; ++id)
        if (!secs.count(id)) throw Fail{"zkey: missing section " + std::to_string(id)};
    auto sized = [&](uint32_t id, uint64_t want, const char* what) {
        if (secs[id].size != want)
            throw Fail{"zkey: section " + std::to_string(id) + " (" + what + ") has " + std::to_string(secs[id].size) + " bytes, " +
                       std::to_string(want) + " expected"};
        return d + secs[id].off;
    };
    // -- section 1
    const uint32_t protocol = rd32(sized(1, 4, "protocol"));
    if (protocol == 2) throw Fail{"zkey: PLONK keys (protocol 2) are not supported: Groth16 only"};
    if (protocol == 10) throw Fail{"zkey: fflonk keys (protocol 10) are not supported: Groth16 only"};
    if (protocol != 1) throw Fail{"zkey: unknown protocol " + std::to_string(protocol) + " (1 = Groth16 expected)"};
    // -- section 2
    if (secs[2].size < 4 || rd32(d + secs[2].off) != 32)
        throw Fail{"zkey: n8q is not 32 (only BN254 is supported)"};
    if (secs[2].size < 72 || rd32(d + secs[2].off + 36) != 32) throw Fail{"zkey: n8r is not 32 (only BN254 is supported)"};
    const uint8_t* h = sized(2, SEC_HEADER_BYTES, "header");
    if (!cwc::u256_eq(rd_fq(h + 4), fq_p())) throw Fail{"zkey: base field q is not BN254's"};
    if (!cwc::u256_eq(rd_fq(h + 40), cwc::fr_p())) throw Fail{"zkey: scalar field r is not BN254's"};
    gwb_zkey_info_t& in = z.info;
    in.n_vars = rd32(h + 72);
    in.n_public = rd32(h + 76);
    in.domain_size = rd32(h + 80);
    if (in.domain_size == 0 || (in.domain_size & (in.domain_size - 1)))
        throw Fail{"zkey: domainSize " + std::to_string(in.domain_size) + " is not a power of two"};
    if ((uint64_t)in.n_public + 1 > in.n_vars) throw Fail{"zkey: nPublic + 1 exceeds nVars"};
    if (in.n_vars > 0x7fffffffu) throw Fail{"zkey: nVars above 2^31 - 1"};
    const uint8_t* pts = h + 84;
    memcpy(z.alpha1, pts, G1_BYTES);
    memcpy(z.beta1, pts + 64, G1_BYTES);
    memcpy(z.beta2, pts + 128, G2_BYTES);
    memcpy(z.gamma2, pts + 256, G2_BYTES);
    memcpy(z.delta1, pts + 384, G1_BYTES);
    memcpy(z.delta2, pts + 448, G2_BYTES);
    check_points("alpha1", z.alpha1, 1, false);
    check_points("beta1", z.beta1, 1, false);
    check_points("beta2", z.beta2, 1, true);
    check_points("gamma2", z.gamma2, 1, true);
    check_points("delta1", z.delta1, 1, false);
    check_points("delta2", z.delta2, 1, true);
    // -- section 4 (bounds only here; the entries are kept, and the witness map is built from them at its first use:
    //    zkey_coefs.cc, which also refuses what a prover cannot use -- values >= r, no entries, a domain the NTT cannot take)
    {
        const uint64_t size = secs[4].size;
        if (size < 4) throw Fail{"zkey: section 4 (coefficients) is truncated"};
        const uint8_t* p = d + secs[4].off;
        in.n_coefs = rd32(p);
        if (size != 4 + in.n_coefs * 44)
            throw Fail{"zkey: section 4 (coefficients) has " + std::to_string(size) + " bytes, " + std::to_string(4 + in.n_coefs * 44) +
                       " expected for " + std::to_string(in.n_coefs) + " coefficients"};
        for (uint64_t k = 0; k < in.n_coefs; ++k) {
            const uint8_t* e = p + 4 + k * 44;
            if (rd32(e) > 1) throw Fail{"zkey: coefficient " + std::to_string(k) + " names matrix " + std::to_string(rd32(e))};
            if (rd32(e + 4) >= in.domain_size) throw Fail{"zkey: coefficient " + std::to_string(k) + " names a constraint >= domainSize"};
            if (rd32(e + 8) >= in.n_vars) throw Fail{"zkey: coefficient " + std::to_string(k) + " names a signal >= nVars"};
        }
        z.sec4.assign(p + 4, p + size);
    }
    // -- point sections
    struct PS {
        uint32_t id;
        uint64_t n;
        bool g2;
        const char* what;
        std::vector<uint8_t>* dst;
    };
    const PS ps[] = {{3, (uint64_t)in.n_public + 1, false, "IC", &z.ic},
                     {5, in.n_vars, false, "A", &z.a},
                     {6, in.n_vars, false, "B1", &z.b1},
                     {7, in.n_vars, true, "B2", &z.b2},
                     {8, (uint64_t)in.n_vars - in.n_public - 1, false, "C", &z.c},
                     {9, in.domain_size, false, "H", &z.h}};
    for (const PS& s : ps) {
        const uint8_t* p = sized(s.id, s.n * (s.g2 ? G2_BYTES : G1_BYTES), s.what);
        check_points(s.what, p, s.n, s.g2);
        s.dst->assign(p, p + secs[s.id].size);
    }
}

}  // namespace

extern "C" {

int gwb_zkey_load(const void* data, size_t len, gwb_zkey_t** out, gw_status_t* status) {
    if (!out || (!data && len)) {
        cwc_r1cs::set_status(status, "gwb_zkey_load: NULL argument");
        return 1;
    }
    *out = nullptr;
    gwb_zkey* z = new gwb_zkey();
    try {
        load((const uint8_t*)data, len, *z);
    } catch (const Fail& f) {
        delete z;
        cwc_r1cs::set_status(status, f.msg);
        return 1;
    } catch (const std::bad_alloc&) {
        delete z;
        cwc_r1cs::set_status(status, "zkey: out of host memory");
        return 1;
    }
    *out = z;
    cwc_r1cs::set_ok(status);
    return 0;
}

int gwb_zkey_check_wtns(const gwb_zkey_t* z, const void* wtns, size_t wtns_len, gw_status_t* status) {
    if (!z || (!wtns && wtns_len)) return cwc_r1cs::fail(status, "gwb_zkey_check_wtns: NULL argument");
    const uint8_t* values = nullptr;
    uint64_t n_wit = 0;
    std::string err;
    if (!cwc_r1cs::parse_wtns(wtns, wtns_len, &values, &n_wit, err)) return cwc_r1cs::fail(status, err);
    if (n_wit != z->info.n_vars)
        return cwc_r1cs::fail(status, "groth16: the witness has " + std::to_string(n_wit) + " elements, the zkey nVars = " + std::to_string(z->info.n_vars));
    cwc_r1cs::set_ok(status);
    return 0;
}

int gwb_zkey_info(const gwb_zkey_t* z, gwb_zkey_info_t* info) {
    if (!z || !info) return 1;
    *info = z->info;
    return 0;
}

}  // extern "C"
