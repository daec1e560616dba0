// What the trapdoor setup (setup.hip, which defines it) and the powers-of-tau setup (setup_ptau.hip) share: the by-wire transpose
// of the constraint matrices on the host and on the device, the order of the key's G1 list, section 4, the conversion to affine
// bytes and the `.zkey` image.  For .hip files.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "groth16_internal.hpp"
#include "hip_util.hpp"

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

// Columns and the handle's coefficients on the device
struct DeviceColumns {
    const uint32_t *ent = nullptr, *cidx = nullptr, *seg_off = nullptr, *seg_key = nullptr, *wire_seg = nullptr;
    const cwc::Fr* coef = nullptr;
    uint32_t n_seg = 0;
};
// Carves the six arrays from the device address `at` on, columns_bytes() in all, and enqueues their upload; an error goes to e,
// and nothing is enqueued once e holds one.
size_t columns_bytes(const Columns& c, size_t n_coef);
DeviceColumns upload_columns(const Columns& c, const std::vector<cwc::Fr>& coef, uint8_t* at, hipStream_t s, hipError_t& e);

// The order of the key's G1 points and of the scalars they come from: [A: nW][B1: nW][C: nW - nPub - 1][H: n][IC: nPub + 1], then
// what the setup appends (the header's points).  A starts at 0.
struct KeyLayout {
    uint32_t n_wires, n_pub, n;
    FRD size_t b1() const { return n_wires; }
    FRD size_t c() const { return 2 * (size_t)n_wires; }
    FRD size_t h() const { return c() + (n_wires - n_pub - 1); }
    FRD size_t ic() const { return h() + n; }
    FRD size_t n1() const { return ic() + n_pub + 1; }  // 3 nW + n
};

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
