// A parsed `.ptau` (ptau.cc), for the powers-of-tau setup (setup_ptau.hip) and the G2 subgroup check (subgroup.hip).  What the
// two key setups share is in setup_internal.hpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "binfile.hpp"
#include "bn254_points_gfx950.hpp"
#include "groth16_internal.hpp"

namespace cwc_ptau {

constexpr uint32_t MAX_SECTION = 15;
constexpr uint32_t MAX_POWER = 28;

// Header and section table of a `.ptau` image; the pointers are into the caller's bytes (an mmap'd file is fine).
struct View {
    uint32_t power = 0, ceremony_power = 0, n_contributions = 0;
    bool prepared = false;  // sections 12 to 15 are present with the sizes of `powersoftau prepare phase2`
    cwc_r1cs::BinSection sec[MAX_SECTION + 1];
};

// What a setup for the domain 2^p reads.  Monomial prefixes: t1 (2n points), t2, at, bt (n each); they are read in full only
// when `from_file` is false, else their first point alone.  Lagrange forms (from_file): l1, l2, la, lb (n each, level p) and
// m (2n points, level p + 1 of section 12, of which the odd ones are read).
struct Plan {
    uint32_t p = 0;
    bool from_file = false;
    const uint8_t *t1 = nullptr, *t2 = nullptr, *at = nullptr, *bt = nullptr, *beta2 = nullptr;
    const uint8_t *l1 = nullptr, *l2 = nullptr, *la = nullptr, *lb = nullptr, *m = nullptr;
};

// header, section table, sizes of the required sections, T1_0 = G1, T2_0 = G2, section 6's point
bool parse(const uint8_t* d, size_t len, View& v, std::string& err);
// mode: GWB_PTAU_LAGRANGE_*; refuses p + 1 > power and `file` without prepared sections
bool plan(const View& v, uint32_t p, uint32_t mode, Plan& pl, std::string& err);
// every point the plan reads other than the bulk arrays' (alpha1, beta1): host check
bool check_header_points(const Plan& pl, std::string& err);
// the bulk arrays, on the host (gwb_ptau_check; the setup checks them on the device)
bool check_bulk_points(const Plan& pl, std::string& err);
// "ptau: section 2 (tauG1) point 5 is not on the G1 curve"; SUBGROUP (subgroup.hip, G2 only): "... is not in the order-r subgroup
// of G2"; NONE, which no caller should reach, says that host and device disagree
std::string point_message(uint32_t section, uint64_t index, cwc_g16::PointFault fault, bool g2);

}  // namespace cwc_ptau
