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
// delta2 and section 7 on the device when asked (Groth16(zkey, check_g2=True), groth16-prove --check-g2).  The section table is
// read by binfile.hpp, the points are checked by the host build of bn254_points_gfx950.hpp.
#include <string.h>

#include <string>

#include "binfile.hpp"
#include "bn254_points_gfx950.hpp"
#include "groth16_internal.hpp"

using namespace cwc_g16;
using cwc_r1cs::BinSection;
using cwc_r1cs::binfile_sections;
using cwc_r1cs::rd32;

namespace {

struct Fail {
    std::string msg;
};

constexpr uint32_t SEC_HEADER_BYTES = 4 + 32 + 4 + 32 + 12 + 3 * G1_BYTES + 3 * G2_BYTES;  // 660

// n points at p: coordinates below q, on the curve unless all zero (bn254_points_gfx950.hpp's point_fault)
void require_points(const char* what, const uint8_t* p, uint64_t n, bool g2) {
    for (uint64_t i = 0; i < n; ++i) {
        const PointFault f = g2 ? point_fault<G2>(p + i * G2_BYTES, false) : point_fault<G1>(p + i * G1_BYTES, false);
        if (f == PointFault::COORDINATE) throw Fail{std::string("zkey: ") + what + " point " + std::to_string(i) + " has a coordinate >= q"};
        if (f == PointFault::CURVE) throw Fail{std::string("zkey: ") + what + " point " + std::to_string(i) + " is not on the " + (g2 ? "G2" : "G1") + " curve"};
    }
}

void load(const uint8_t* d, size_t len, gwb_zkey& z) {
    BinSection secs[11];
    std::string err;
    if (!binfile_sections(d, len, "zkey", 0x7feu, secs, err)) throw Fail{err};  // sections 1 to 10
    for (uint32_t id = 1; id <= 9; ++id)
        if (!secs[id].p) throw Fail{"zkey: missing section " + std::to_string(id)};
    auto sized = [&](uint32_t id, uint64_t want, const char* what) {
        if (secs[id].size != want)
            throw Fail{"zkey: section " + std::to_string(id) + " (" + what + ") has " + std::to_string(secs[id].size) + " bytes, " +
                       std::to_string(want) + " expected"};
        return secs[id].p;
    };
    // -- section 1
    const uint32_t protocol = rd32(sized(1, 4, "protocol"));
    if (protocol == 2) throw Fail{"zkey: PLONK keys (protocol 2) are not supported: Groth16 only"};
    if (protocol == 10) throw Fail{"zkey: fflonk keys (protocol 10) are not supported: Groth16 only"};
    if (protocol != 1) throw Fail{"zkey: unknown protocol " + std::to_string(protocol) + " (1 = Groth16 expected)"};
    // -- section 2
    if (secs[2].size < 4 || rd32(secs[2].p) != 32)
        throw Fail{"zkey: n8q is not 32 (only BN254 is supported)"};
    if (secs[2].size < 72 || rd32(secs[2].p + 36) != 32) throw Fail{"zkey: n8r is not 32 (only BN254 is supported)"};
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
    require_points("alpha1", z.alpha1, 1, false);
    require_points("beta1", z.beta1, 1, false);
    require_points("beta2", z.beta2, 1, true);
    require_points("gamma2", z.gamma2, 1, true);
    require_points("delta1", z.delta1, 1, false);
    require_points("delta2", z.delta2, 1, true);
    // -- section 4 (bounds only here; the entries are kept, and the witness map is built from them at its first use:
    //    zkey_coefs.cc, which also refuses what a prover cannot use -- values >= r, no entries, a domain the NTT cannot take)
    {
        const uint64_t size = secs[4].size;
        if (size < 4) throw Fail{"zkey: section 4 (coefficients) is truncated"};
        const uint8_t* p = secs[4].p;
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
        require_points(s.what, p, s.n, s.g2);
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
