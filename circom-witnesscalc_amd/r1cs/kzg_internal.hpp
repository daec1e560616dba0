// What kzg.cc (the handle, the C ABI) asks of kzg.hip (the kernels and their launches): include/graph_witness_kzg.h has the
// definitions.  Everything here is asynchronous on the caller's stream and takes device addresses.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

namespace cwc_kzg {

constexpr uint32_t TILE_SMALL = 256, TILE_PRODUCTION = 1024;  // coefficients per workgroup, the instantiated sizes
constexpr uint32_t PENDING = 0xffffffffu;                      // a row's status while its pairings decide
constexpr uint32_t MAX_PAIRS_PER_LAUNCH = 32768;               // the pair index is the grid's second dimension

inline bool tile_ok(uint32_t tile) { return tile == TILE_SMALL || tile == TILE_PRODUCTION; }

// Bytes of the levels' workspace of enqueue_eval_quotient for K pairs of N coefficients (the points z^(tile^l), the tile totals
// and the carries of every level above the first; the quotients themselves are the caller's).
size_t eval_quotient_ws(uint64_t K, uint64_t N, uint32_t tile);
// d_polys [K][N][32], d_zs [K / z_div][32] (pair i takes point i / z_div: 1, or the polynomials per group of a folded opening)
// -> d_ys [K][32] and, unless d_qs is null, d_qs [K][N - 1][32]; canonical.  N >= 1.
bool enqueue_eval_quotient(const uint8_t* d_polys, const uint8_t* d_zs, uint32_t z_div, uint64_t K, uint32_t N, uint32_t tile, uint8_t* d_ys, uint8_t* d_qs,
                           uint8_t* d_ws, hipStream_t s, std::string& err);
// Per opening: the scalar and point rules, L = C - y G1 + z W, and the pairing inputs (L, G2), (W, tauG2) at the rows 2i, 2i + 1 of
// d_g1 [2K][64] and d_g2 [2K][128]; d_status[i] is a verdict or PENDING (then the generators stand in both rows).
bool enqueue_prepare(const uint8_t* d_c, const uint8_t* d_z, const uint8_t* d_y, const uint8_t* d_w, uint32_t K, const uint8_t* d_tau_g2, uint8_t* d_g1,
                     uint8_t* d_g2, uint32_t* d_status, hipStream_t s, std::string& err);
// PENDING rows: VALID when d_gt[2i] and d_gt[2i + 1] have equal bytes, else EQUATION
bool enqueue_compare(const uint8_t* d_gt, uint32_t K, uint32_t* d_status, hipStream_t s, std::string& err);

// Folded openings: G groups of K polynomials (or points) each, one gamma per group.
constexpr uint64_t MAX_FOLD_PAIRS = 0x7fffffffu;  // G K: a pair's index, and a group's term index K + 1, are 32-bit in the kernels
constexpr size_t FOLD_PARTIAL_BYTES = 132;        // the point fold's workspace per group and chunk of 64 terms: an XYZZ sum and its flags
// d_polys [G][K][N][32], d_gammas [G][32], any values -> d_out [G][N][32] = sum_k gamma^k p_k, canonical.  K, N >= 1.
bool enqueue_fold(const uint8_t* d_polys, const uint8_t* d_gammas, uint64_t G, uint32_t K, uint32_t N, uint8_t* d_out, hipStream_t s, std::string& err);
// The point fold's partial sums into d_ws (fold_points_ws bytes, for the same G as the call that reads them).  Without d_w:
// sum_k gamma^k C_k per group, gamma reduced.  With d_w, the verifier's L = sum_k gamma^k C_k - y_f G1 + z W and its scalar and point rules.
size_t fold_points_ws(uint64_t G, uint32_t K, bool check);
bool enqueue_fold_points(const uint8_t* d_c, const uint8_t* d_gammas, const uint8_t* d_z, const uint8_t* d_y, const uint8_t* d_w, uint64_t G, uint32_t K,
                         uint8_t* d_ws, hipStream_t s, std::string& err);
// enqueue_prepare's outputs for G groups, from the partial sums of enqueue_fold_points with d_w
bool enqueue_fold_emit(const uint8_t* d_ws, const uint8_t* d_w, uint32_t G, uint32_t K, const uint8_t* d_tau_g2, uint8_t* d_g1, uint8_t* d_g2, uint32_t* d_status,
                       hipStream_t s, std::string& err);
// d_out [G][64] canonical from the partial sums of enqueue_fold_points without d_w; *d_fault = min(*d_fault, the first group with a refused point)
bool enqueue_fold_sum(const uint8_t* d_ws, uint32_t G, uint32_t K, uint8_t* d_out, uint32_t* d_fault, hipStream_t s, std::string& err);

}  // namespace cwc_kzg
