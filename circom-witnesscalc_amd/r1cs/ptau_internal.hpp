// A parsed `.ptau` (ptau.cc) and the pieces of the trapdoor setup (setup.hip) that the powers-of-tau setup (setup_ptau.hip)
// shares with it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "groth16_internal.hpp"

namespace cwc_ptau {

constexpr uint32_t MAX_SECTION = 15;
constexpr uint32_t MAX_POWER = 28;

// Header and section table of a `.ptau` image; the pointers are into the caller's bytes (an mmap'd file is fine).
struct View {
    uint32_t power = 0, ceremony_power = 0, n_contributions = 0;
    bool prepared = false;  // sections 12 to 15 are present with the sizes of `powersoftau prepare phase2`
    const uint8_t* sec[MAX_SECTION + 1] = {};
    uint64_t size[MAX_SECTION + 1] = {};
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

enum PointFault : uint32_t { COORDINATE = 0, CURVE = 1, SUBGROUP = 2 };

// header, section table, sizes of the required sections, T1_0 = G1, T2_0 = G2, section 6's point
bool parse(const uint8_t* d, size_t len, View& v, std::string& err);
// mode: GWB_PTAU_LAGRANGE_*; refuses p + 1 > power and `file` without prepared sections
bool plan(const View& v, uint32_t p, uint32_t mode, Plan& pl, std::string& err);
// every point the plan reads other than the bulk arrays' (alpha1, beta1): host check
bool check_header_points(const Plan& pl, std::string& err);
// the bulk arrays, on the host (gwb_ptau_check; the setup checks them on the device)
bool check_bulk_points(const Plan& pl, std::string& err);
// "ptau: section 2 (tauG1) point 5 is not on the G1 curve"; SUBGROUP (subgroup.hip, G2 only): "... is not in the order-r subgroup of G2"
std::string point_message(uint32_t section, uint64_t index, uint32_t fault, bool g2);

}  // namespace cwc_ptau

// setup.hip
namespace cwc_setup {

// The by-wire transpose of the handle's matrices: the terms of column (wire, matrix), key 3 wire + matrix, in key order.
struct Columns {
    std::vector<uint32_t> ent, cidx;         // per term: constraint (file index) | kind << 30; coefficient index
    std::vector<uint32_t> seg_off, seg_key;  // segments: terms seg_off[s] .. seg_off[s + 1] of column seg_key[s]
    std::vector<uint32_t> wire_seg;          // wire i's segments: wire_seg[i] .. wire_seg[i + 1]
};
void transpose(const gwb_r1cs* r, uint32_t segment, Columns& c);
uint32_t segment_terms();  // CWC_GROTH16_SETUP_SEGMENT or 64
bool coefficients_section(const gwb_r1cs* r, std::vector<uint8_t>& out, std::string& err);

// the generators as the files store them (affine, Montgomery form): 64 and 128 bytes
void generator_bytes(uint8_t* g1, uint8_t* g2);

// XYZZ points on the device -> affine bytes (Montgomery as the zkey stores them, or canonical), shared inversions
void enqueue_affine_g1(const void* d_xyzz, uint32_t n, uint8_t* d_out, bool canonical, void* stream);
void enqueue_affine_g2(const void* d_xyzz, uint32_t n, uint8_t* d_out, bool canonical, void* stream);

// The `.zkey` image: sections 1 to 10 in ascending order, section 10 without hash or contributions.  Points as stored.
struct KeyPoints {
    uint32_t n_wires, n_pub, n;
    const uint8_t *alpha1, *beta1, *beta2, *gamma2, *delta1, *delta2;
    const uint8_t *ic, *a, *b1, *b2, *c, *h;
};
int write_zkey(const KeyPoints& k, const std::vector<uint8_t>& sec4, void** zkey, size_t* zkey_len, gw_status_t* status);

}  // namespace cwc_setup
