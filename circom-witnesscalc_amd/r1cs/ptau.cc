// `.ptau` loader (iden3 binfile "ptau" version 1, a powers-of-tau ceremony file as snarkjs writes it): hostile bytes in, a
// validated view or a message out.  All integers little-endian; sections in any order; unknown sections are passed over.
// Points are affine, uncompressed, every coordinate 32 bytes in Montgomery form mod q (R = 2^256), as in the zkey.
//   file:       "ptau", u32 version = 1, u32 nSections, then per section u32 id, u64 size, size bytes
//   section 1:  u32 n8 = 32, q, u32 power, u32 ceremonyPower
//   section 2:  tauG1, 2^(power+1) - 1 G1      section 3: tauG2, 2^power G2
//   section 4:  alphaTauG1, 2^power G1         section 5: betaTauG1, 2^power G1       section 6: betaG2, one G2
//   section 7:  u32 nContributions, then the contribution records (not read)
//   sections 12 to 15 (optional, `powersoftau prepare phase2`): the Lagrange forms of sections 2 to 5; level m (the 2^m points
//   Lag_m of the first 2^m monomial points) starts at point offset 2^m - 1; levels 0 .. power, and in section 12 also power + 1.
// The loader reads the header, the section table, and of the points only what a setup for one domain needs (Plan): it never
// walks a whole section, so a file of gigabytes that is mapped into memory is touched in a few places.  G2 points are not
// checked for subgroup membership here; gwb_ptau_check_g2 (subgroup.hip) checks those a setup reads, on the device, when asked
// (groth16_setup_ptau(..., check_g2=True), groth16-setup --ptau FILE --check-g2).  The layout is restated from snarkjs's writer; no snarkjs output was available to check it.
#include <string.h>

#include <string>

#include "../../include/graph_witness_groth16_ptau.h"
#include "fq_gfx950.hpp"
#include "ptau_internal.hpp"

using namespace cwc_g16;

namespace cwc_ptau {

namespace {

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

const char* section_name(uint32_t id) {
    static const char* names[MAX_SECTION + 1] = {"", "header", "tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2", "contributions",
                                                 "", "", "", "", "lagrange tauG1", "lagrange tauG2", "lagrange alphaTauG1", "lagrange betaTauG1"};
    return id <= MAX_SECTION ? names[id] : "";
}

// n points at p, every `stride`-th from `first`: coordinates below q, on the curve unless all zero
bool check_points(uint32_t section, const uint8_t* p, uint64_t base_index, uint64_t n, uint64_t first, uint64_t stride, bool g2, std::string& err) {
    const Fq b1 = fq_to_mont(Fq{{3, 0, 0, 0, 0, 0, 0, 0}});
    static const Fq2 b2 = g2_b();
    const uint32_t words = g2 ? 4 : 2;
    for (uint64_t i = first; i < n; i += stride) {
        const uint8_t* pt = p + i * words * 32;
        bool zero = true;
        for (uint32_t k = 0; k < words; ++k) {
            const Fq c = rd_fq(pt + 32 * k);
            if (!cwc::u256_lt(c, fq_p())) {
                err = point_message(section, base_index + i, COORDINATE, g2);
                return false;
            }
            zero = zero && cwc::u256_is_zero(c);
        }
        if (zero) continue;
        const bool ok = g2 ? on_curve<Fq2T>(Affine<Fq2T>{Fq2{rd_fq(pt), rd_fq(pt + 32)}, Fq2{rd_fq(pt + 64), rd_fq(pt + 96)}}, b2)
                           : on_curve<FqT>(Affine<FqT>{rd_fq(pt), rd_fq(pt + 32)}, b1);
        if (!ok) {
            err = point_message(section, base_index + i, CURVE, g2);
            return false;
        }
    }
    return true;
}

}  // namespace

std::string point_message(uint32_t section, uint64_t index, uint32_t fault, bool g2) {
    std::string m = "ptau: section " + std::to_string(section) + " (" + section_name(section) + ") point " + std::to_string(index);
    if (fault == SUBGROUP) return m + " is not in the order-r subgroup of G2";
    return m + (fault == COORDINATE ? " has a coordinate >= q" : std::string(" is not on the ") + (g2 ? "G2" : "G1") + " curve");
}

bool parse(const uint8_t* d, size_t len, View& v, std::string& err) {
    if (len < 12 || memcmp(d, "ptau", 4) != 0) {
        err = "ptau: bad magic (not a .ptau file)";
        return false;
    }
    const uint32_t version = rd32(d + 4), n_sections = rd32(d + 8);
    if (version != 1) {
        err = "ptau: unsupported version " + std::to_string(version) + " (1 expected)";
        return false;
    }
    uint64_t off = 12;
    for (uint32_t i = 0; i < n_sections; ++i) {
        if (len - off < 12) {
            err = "ptau: truncated section header";
            return false;
        }
        const uint32_t id = rd32(d + off);
        uint64_t size;
        memcpy(&size, d + off + 4, 8);
        off += 12;
        if (size > len - off) {
            err = "ptau: truncated section " + std::to_string(id) + " (declares " + std::to_string(size) + " bytes, " + std::to_string(len - off) +
                  " left)";
            return false;
        }
        if ((id >= 1 && id <= 7) || (id >= 12 && id <= 15)) {
            if (v.sec[id]) {
                err = "ptau: duplicate section " + std::to_string(id);
                return false;
            }
            v.sec[id] = d + off;
            v.size[id] = size;
        }
        off += size;
    }
    if (off != len) {
        err = "ptau: " + std::to_string(len - off) + " trailing bytes after the last section";
        return false;
    }
    for (uint32_t id = 1; id <= 6; ++id)
        if (!v.sec[id]) {
            err = "ptau: missing section " + std::to_string(id) + " (" + section_name(id) + ")";
            return false;
        }
    // -- section 1
    if (v.size[1] < 4 || rd32(v.sec[1]) != 32) {
        err = "ptau: n8 is not 32 (only BN254 is supported)";
        return false;
    }
    auto sized = [&](uint32_t id, uint64_t want) {
        if (v.size[id] == want) return true;
        err = "ptau: section " + std::to_string(id) + " (" + section_name(id) + ") has " + std::to_string(v.size[id]) + " bytes, " +
              std::to_string(want) + " expected";
        return false;
    };
    if (!sized(1, 44)) return false;
    if (!cwc::u256_eq(rd_fq(v.sec[1] + 4), fq_p())) {
        err = "ptau: base field q is not BN254's";
        return false;
    }
    v.power = rd32(v.sec[1] + 36);
    v.ceremony_power = rd32(v.sec[1] + 40);
    if (v.power > MAX_POWER) {
        err = "ptau: power " + std::to_string(v.power) + " is above " + std::to_string(MAX_POWER);
        return false;
    }
    const uint64_t np = 1ull << v.power;
    if (!sized(2, (2 * np - 1) * G1_BYTES) || !sized(3, np * G2_BYTES) || !sized(4, np * G1_BYTES) || !sized(5, np * G1_BYTES) ||
        !sized(6, G2_BYTES))
        return false;
    v.n_contributions = v.sec[7] && v.size[7] >= 4 ? rd32(v.sec[7]) : 0;
    v.prepared = v.sec[12] && v.sec[13] && v.sec[14] && v.sec[15] && v.size[12] == (4 * np - 1) * G1_BYTES &&
                 v.size[13] == (2 * np - 1) * G2_BYTES && v.size[14] == (2 * np - 1) * G1_BYTES && v.size[15] == (2 * np - 1) * G1_BYTES;
    // -- the generators
    uint8_t g1[G1_BYTES], g2[G2_BYTES];
    cwc_setup::generator_bytes(g1, g2);
    if (memcmp(v.sec[2], g1, G1_BYTES) != 0) {
        err = "ptau: section 2 (tauG1) point 0 is not the G1 generator";
        return false;
    }
    if (memcmp(v.sec[3], g2, G2_BYTES) != 0) {
        err = "ptau: section 3 (tauG2) point 0 is not the G2 generator";
        return false;
    }
    return true;
}

bool plan(const View& v, uint32_t p, uint32_t mode, Plan& pl, std::string& err) {
    if (mode > GWB_PTAU_LAGRANGE_COMPUTE) {
        err = "ptau: lagrange mode " + std::to_string(mode) + " (0 = auto, 1 = file, 2 = compute expected)";
        return false;
    }
    if (p + 1 > v.power) {
        err = "ptau: the circuit's domain 2^" + std::to_string(p) + " needs a ceremony of power " + std::to_string(p + 1) + " or more, this file has power " +
              std::to_string(v.power) + " (the truncated top level that snarkjs accepts for 2^power is not supported)";
        return false;
    }
    if (mode == GWB_PTAU_LAGRANGE_FILE && !v.prepared) {
        err = "ptau: lagrange = file, but the file has no prepared sections 12 to 15 (run `powersoftau prepare phase2`, or use auto or compute)";
        return false;
    }
    pl.p = p;
    pl.from_file = mode == GWB_PTAU_LAGRANGE_FILE || (mode == GWB_PTAU_LAGRANGE_AUTO && v.prepared);
    pl.t1 = v.sec[2];
    pl.t2 = v.sec[3];
    pl.at = v.sec[4];
    pl.bt = v.sec[5];
    pl.beta2 = v.sec[6];
    if (pl.from_file) {
        const uint64_t n = 1ull << p, lvl = n - 1, lvl2 = 2 * n - 1;
        pl.l1 = v.sec[12] + lvl * G1_BYTES;
        pl.l2 = v.sec[13] + lvl * G2_BYTES;
        pl.la = v.sec[14] + lvl * G1_BYTES;
        pl.lb = v.sec[15] + lvl * G1_BYTES;
        pl.m = v.sec[12] + lvl2 * G1_BYTES;
    }
    return true;
}

bool check_header_points(const Plan& pl, std::string& err) {
    return check_points(4, pl.at, 0, 1, 0, 1, false, err) && check_points(5, pl.bt, 0, 1, 0, 1, false, err) &&
           check_points(6, pl.beta2, 0, 1, 0, 1, true, err);
}

bool check_bulk_points(const Plan& pl, std::string& err) {
    const uint64_t n = 1ull << pl.p;
    if (pl.from_file)
        return check_points(12, pl.l1, n - 1, n, 0, 1, false, err) && check_points(13, pl.l2, n - 1, n, 0, 1, true, err) &&
               check_points(14, pl.la, n - 1, n, 0, 1, false, err) && check_points(15, pl.lb, n - 1, n, 0, 1, false, err) &&
               check_points(12, pl.m, 2 * n - 1, 2 * n, 1, 2, false, err);
    return check_points(2, pl.t1, 0, 2 * n, 0, 1, false, err) && check_points(3, pl.t2, 0, n, 0, 1, true, err) &&
           check_points(4, pl.at, 0, n, 0, 1, false, err) && check_points(5, pl.bt, 0, n, 0, 1, false, err);
}

}  // namespace cwc_ptau

extern "C" {

int gwb_ptau_info(const void* data, size_t len, gwb_ptau_info_t* info, gw_status_t* status) {
    if (!info || (!data && len)) return cwc_r1cs::fail(status, "gwb_ptau_info: NULL argument");
    cwc_ptau::View v;
    std::string err;
    if (!cwc_ptau::parse((const uint8_t*)data, len, v, err)) return cwc_r1cs::fail(status, err);
    info->power = v.power;
    info->ceremony_power = v.ceremony_power;
    info->prepared = v.prepared ? 1 : 0;
    info->n_contributions = v.n_contributions;
    cwc_r1cs::set_ok(status);
    return 0;
}

int gwb_ptau_check(const void* data, size_t len, uint32_t domain_power, uint32_t lagrange_mode, gw_status_t* status) {
    if (!data && len) return cwc_r1cs::fail(status, "gwb_ptau_check: NULL argument");
    cwc_ptau::View v;
    cwc_ptau::Plan pl;
    std::string err;
    if (!cwc_ptau::parse((const uint8_t*)data, len, v, err) || !cwc_ptau::plan(v, domain_power, lagrange_mode, pl, err) ||
        !cwc_ptau::check_header_points(pl, err) || !cwc_ptau::check_bulk_points(pl, err))
        return cwc_r1cs::fail(status, err);
    cwc_r1cs::set_ok(status);
    return 0;
}

}  // extern "C"
