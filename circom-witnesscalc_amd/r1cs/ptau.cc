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
#include "binfile.hpp"
#include "bn254_points_gfx950.hpp"
#include "ptau_internal.hpp"

using namespace cwc_g16;
using cwc_r1cs::rd32;

namespace cwc_ptau {

const char* section_name(uint32_t id) {
    static const char* names[MAX_SECTION + 1] = {"", "header", "tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2", "contributions",
                                                 "", "", "", "", "lagrange tauG1", "lagrange tauG2", "lagrange alphaTauG1", "lagrange betaTauG1"};
    return id <= MAX_SECTION ? names[id] : "";
}

namespace {

// n points at p, every `stride`-th from `first`: coordinates below q, on the curve unless all zero
bool check_points(uint32_t section, const uint8_t* p, uint64_t base_index, uint64_t n, uint64_t first, uint64_t stride, bool g2, std::string& err) {
    for (uint64_t i = first; i < n; i += stride) {
        const PointFault f = g2 ? point_fault<G2>(p + i * G2_BYTES, false) : point_fault<G1>(p + i * G1_BYTES, false);
        if (f == PointFault::NONE) continue;
        err = point_message(section, base_index + i, f, g2);
        return false;
    }
    return true;
}

}  // namespace

std::string point_message(uint32_t section, uint64_t index, PointFault fault, bool g2) {
    std::string m = "ptau: section " + std::to_string(section) + " (" + section_name(section) + ") point " + std::to_string(index);
    switch (fault) {
        case PointFault::COORDINATE: return m + " has a coordinate >= q";
        case PointFault::CURVE: return m + " is not on the " + (g2 ? "G2" : "G1") + " curve";
        case PointFault::SUBGROUP: return m + " is not in the order-r subgroup of G2";
        case PointFault::NONE: break;
    }
    return m + " was refused by the device, and the host finds no fault in it";
}

bool parse(const uint8_t* d, size_t len, View& v, std::string& err) {
    if (!cwc_r1cs::binfile_sections(d, len, "ptau", 0xf0feu, v.sec, err, &v.order)) return false;  // sections 1 to 7 and 12 to 15
    for (uint32_t id = 1; id <= 6; ++id)
        if (!v.sec[id].p) {
            err = "ptau: missing section " + std::to_string(id) + " (" + section_name(id) + ")";
            return false;
        }
    // -- section 1
    if (v.sec[1].size < 4 || rd32(v.sec[1].p) != 32) {
        err = "ptau: n8 is not 32 (only BN254 is supported)";
        return false;
    }
    auto sized = [&](uint32_t id, uint64_t want) {
        if (v.sec[id].size == want) return true;
        err = "ptau: section " + std::to_string(id) + " (" + section_name(id) + ") has " + std::to_string(v.sec[id].size) + " bytes, " +
              std::to_string(want) + " expected";
        return false;
    };
    if (!sized(1, 44)) return false;
    if (!cwc::u256_eq(rd_fq(v.sec[1].p + 4), fq_p())) {
        err = "ptau: base field q is not BN254's";
        return false;
    }
    v.power = rd32(v.sec[1].p + 36);
    v.ceremony_power = rd32(v.sec[1].p + 40);
    if (v.power > MAX_POWER) {
        err = "ptau: power " + std::to_string(v.power) + " is above " + std::to_string(MAX_POWER);
        return false;
    }
    const uint64_t np = 1ull << v.power;
    if (!sized(2, (2 * np - 1) * G1_BYTES) || !sized(3, np * G2_BYTES) || !sized(4, np * G1_BYTES) || !sized(5, np * G1_BYTES) ||
        !sized(6, G2_BYTES))
        return false;
    v.n_contributions = v.sec[7].p && v.sec[7].size >= 4 ? rd32(v.sec[7].p) : 0;
    v.prepared = v.sec[12].p && v.sec[13].p && v.sec[14].p && v.sec[15].p && v.sec[12].size == (4 * np - 1) * G1_BYTES &&
                 v.sec[13].size == (2 * np - 1) * G2_BYTES && v.sec[14].size == (2 * np - 1) * G1_BYTES && v.sec[15].size == (2 * np - 1) * G1_BYTES;
    // -- the generators
    uint8_t g1[G1_BYTES], g2[G2_BYTES];
    put_coords<G1>(g1, g1_generator().x, g1_generator().y, false);
    put_coords<G2>(g2, g2_generator().x, g2_generator().y, false);
    if (memcmp(v.sec[2].p, g1, G1_BYTES) != 0) {
        err = "ptau: section 2 (tauG1) point 0 is not the G1 generator";
        return false;
    }
    if (memcmp(v.sec[3].p, g2, G2_BYTES) != 0) {
        err = "ptau: section 3 (tauG2) point 0 is not the G2 generator";
        return false;
    }
    return true;
}

bool need_prepared(const View& v, std::string& err) {
    if (v.prepared) return true;
    err = "ptau: lagrange = file, but the file has no prepared sections 12 to 15 (run `powersoftau prepare phase2`, or use auto or compute)";
    return false;
}

bool check_lagrange_points(const View& v, uint32_t id, uint32_t m_lo, uint32_t m_hi, std::string& err) {
    const bool g2 = id == 13;
    const uint64_t lo = (1ull << m_lo) - 1, hi = (2ull << m_hi) - 1, bytes = g2 ? G2_BYTES : G1_BYTES;
    const uint64_t prefix = (1ull << m_hi) - (id == 12 && m_hi == v.power + 1 ? 1 : 0);
    return check_points(id, v.sec[id].p + lo * bytes, lo, hi - lo, 0, 1, g2, err) && check_points(id - 10, v.sec[id - 10].p, 0, prefix, 0, 1, g2, err);
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
    if (mode == GWB_PTAU_LAGRANGE_FILE && !need_prepared(v, err)) return false;
    pl.p = p;
    pl.from_file = mode == GWB_PTAU_LAGRANGE_FILE || (mode == GWB_PTAU_LAGRANGE_AUTO && v.prepared);
    pl.t1 = v.sec[2].p;
    pl.t2 = v.sec[3].p;
    pl.at = v.sec[4].p;
    pl.bt = v.sec[5].p;
    pl.beta2 = v.sec[6].p;
    if (pl.from_file) {
        const uint64_t n = 1ull << p, lvl = n - 1, lvl2 = 2 * n - 1;
        pl.l1 = v.sec[12].p + lvl * G1_BYTES;
        pl.l2 = v.sec[13].p + lvl * G2_BYTES;
        pl.la = v.sec[14].p + lvl * G1_BYTES;
        pl.lb = v.sec[15].p + lvl * G1_BYTES;
        pl.m = v.sec[12].p + lvl2 * G1_BYTES;
    }
    return true;
}

bool check_header_points(const Plan& pl, std::string& err) {
    return check_points(4, pl.at, 0, 1, 0, 1, false, err) && check_points(5, pl.bt, 0, 1, 0, 1, false, err) &&
           check_points(6, pl.beta2, 0, 1, 0, 1, true, err);
}

bool check_all_points(const View& v, std::string& err) {
    const uint64_t n = 1ull << v.power;
    return check_points(2, v.sec[2].p, 0, 2 * n - 1, 0, 1, false, err) && check_points(3, v.sec[3].p, 0, n, 0, 1, true, err) &&
           check_points(4, v.sec[4].p, 0, n, 0, 1, false, err) && check_points(5, v.sec[5].p, 0, n, 0, 1, false, err) &&
           check_points(6, v.sec[6].p, 0, 1, 0, 1, true, err);
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
