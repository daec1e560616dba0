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
    std::vector<cwc_r1cs::BinEntry> order;  // every section in file order, unknown ids included (what gwb_ptau_prepare_phase2 carries)
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
// every point of the monomial sections 2 to 6, on the host (the whole-file check of gwb_ptau_verify)
bool check_all_points(const View& v, std::string& err);
// "ptau: section 2 (tauG1) point 5 is not on the G1 curve"; SUBGROUP (subgroup.hip, G2 only): "... is not in the order-r subgroup
// of G2"; NONE, which no caller should reach, says that host and device disagree
std::string point_message(uint32_t section, uint64_t index, cwc_g16::PointFault fault, bool g2);
// "tauG1", "lagrange alphaTauG1", ...; "" for an id the layout does not name
const char* section_name(uint32_t id);

// ---- the prepared sections 12 to 15 (setup_ptau.hip writes them, contribute.hip checks them) ------------------------------------

// `lagrange = file`'s refusal of a file without prepared sections
bool need_prepared(const View& v, std::string& err);
// The Lagrange section `id` (12 to 15) holds the levels 0 .. top(id) of the monomial section id - 10; top = power, and power + 1
// for section 12, whose last level is Lag of (T_0 .. T_{2n-2}, O) since section 2 ends one point short.
inline uint32_t top_level(const View& v, uint32_t id) { return id == 12 ? v.power + 1 : v.power; }
// Host check (coordinates, curve; point_message's wording) of what a Lagrange check of levels m_lo .. m_hi of section `id`
// reads: those levels, then the first 2^m_hi points of section id - 10 (one fewer for section 12's last level).
bool check_lagrange_points(const View& v, uint32_t id, uint32_t m_lo, uint32_t m_hi, std::string& err);
// subgroup.hip: G2 subgroup membership of n stored points at host address p, on the current device in pieces; they are points
// base .. base + n of `section`.  0, 1 with point_message's text for the first offender, or 2 with what went wrong.
int check_g2_points(uint32_t section, uint64_t base, const uint8_t* p, uint64_t n, std::string& msg);

// All levels of a section lie in one array, level m (2^m points) in the slots [2^m - 1, 2^(m+1) - 1).  Stage s (half = 2^s) of
// the radix-2 transforms of every level m in (s, top] is one launch of 2^top threads.  Thread v has a twiddle index k < 2^s
// and a w in [0, 2^(top-s)); w = 0 is idle, and otherwise w's top bit j gives the level m = s + 1 + j and the bits below it the
// group of 2 half slots, so the decode is a count of leading zeros.  Butterflies of different levels with one k share their
// twiddle w_(2 half)^(-k), and 2^(top-s) - 1 of them do: while that is 63 or more (top - s >= 6), v = k 2^(top-s) + w and the 64
// lanes of a wave have one k (w = 0 costs one lane in 2^(top-s)); in the last five stages v = w 2^s + k and the lanes take
// consecutive k, which are consecutive slots.  The butterfly is on the slots lo and lo + half, lo = 2^m - 1 + grp 2 half + k.
struct LevelButterfly {
    uint32_t m, grp, k;
};
FRD bool level_butterfly(uint32_t v, uint32_t top, uint32_t s, LevelButterfly& b) {
    const uint32_t span = top - s;
    const bool by_k = span >= 6;
    const uint32_t w = by_k ? v & ((1u << span) - 1u) : v >> s;
    if (w == 0) return false;
    const uint32_t j = 31u - (uint32_t)__builtin_clz(w);
    b.k = by_k ? v >> span : v & ((1u << s) - 1u);
    b.m = s + 1 + j;
    b.grp = w - (1u << j);
    return true;
}

}  // namespace cwc_ptau
