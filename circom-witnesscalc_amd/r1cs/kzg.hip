// The device side of the KZG commitments (include/graph_witness_kzg.h has the definitions): evaluation and quotient of a batch
// of polynomials, and the per-opening arithmetic of the verifier.  The commitments and witnesses themselves are linear
// combinations over the stored SRS and go through contribute.hip's kernels (gwb_bn254_g1_lincomb_device, from kzg.cc), the
// pairings through verify.hip's.
//
// Evaluate and divide.  s_i = c_i + z s_{i+1} is a linear recurrence from the top coefficient down; y = s_0 and q_i = s_{i+1}.
// A workgroup of 256 threads owns a tile of TILE consecutive coefficients and computes the tile's own suffix sums
// t_i = sum_{i <= j < tile end} c_j z^(j-i):
//   load      16 bytes per lane and step, consecutive lanes consecutive addresses, into LDS; each thread then reads its run of
//             RUN = TILE / 256 consecutive coefficients (a run is padded by 16 bytes in LDS, so that the lanes of a wave do not
//             all start in one bank).  A value at or above r is reduced here, on the first level.
//   Horner    over the run from its top: h, the run's suffix sum at its first coefficient.  RUN - 1 products.
//   wave      suffix scan of h over the 64 lanes in 6 steps; step d adds z^(RUN 2^d) times the value 2^d lanes up
//             (__shfl_down, eight words).  The multiplier is the same in every lane: one product and one addition per lane.
//   workgroup the four waves' sums go through LDS, and every wave folds those above it (at most 3 products).
// The tile totals B_b = t_(b TILE) obey K_b = B_(b+1) + z^TILE K_(b+1), K_b = s_((b+1) TILE) being what tile b lacks: the same
// recurrence over N / TILE elements at the point z^TILE, and its "quotient" is K.  So the host recurses with two kernel roles and
// no workgroup ever waits for another: "totals" (writes B_b only) on each level until one tile is left, then "apply" from the
// top level down, which takes K_b, forms the lane's carry-in z^(RUN (64 - lane)) K' by square-and-multiply over the scan's
// multipliers (7 products), and runs Horner over the run a second time from that carry: s_i, RUN products.  The results go
// back through LDS and out with 16 bytes per lane and step: q_(i-1) = s_i, and s_0 is y.  About 2 products per coefficient
// and level, as a serial Horner and a serial division have together.
//
// Values stay canonical throughout and only the powers of z are in Montgomery form: the Montgomery product of a canonical value
// and a power in Montgomery form is their canonical product, so nothing is converted on the way in or out (the conversions
// would be two more products per coefficient).  The powers a workgroup needs (z^RUN, z^(RUN 2^d), z^(64 RUN)) come from the
// level's point by squarings inside the workgroup; the levels' points z^(TILE^l) are made per pair by kzg_points_kernel.
//
// TILE = 256 (RUN = 1) exists for the tests: two levels of recursion at 65 537 coefficients.  TILE = 1024 (RUN = 4) is the
// production tile: 36 KB of LDS and 132 registers in "apply", so three workgroups share a CU and the loads of one overlap the
// products of another; 2048 would be 68 KB, past the 64 KB that a kernel gets without asking for more, with the coefficients of
// a run of 8 alone in 64 registers.  A polynomial of 2^28 coefficients is three levels with either.
//
// Opening check.  kzg_prepare_kernel, one thread per opening and one wave per workgroup (the two multiplications of
// xyzz_mul_short want the wave's registers, as mul_points_kernel<G1, 1> does): y, z below r; C, W decoded and checked by
// get_point; L = C - y G1 + z W; the pairing inputs (L, G2), (W, tauG2).  A row that a rule has decided, or whose L or W is the
// point at infinity (the pairing path does not take it), gets its status here and the generators as pairing inputs;
// kzg_compare_kernel sets the others from the GT bytes.
//
// Folded openings (K polynomials of a group at one point under one witness).  kzg_fold_kernel makes f = sum_k gamma^k p_k: one
// thread per coefficient index, Horner in gamma from the last polynomial down, two 16-byte loads per step with consecutive lanes
// on consecutive elements (a wave reads 2 KB contiguously); the same trick as above, canonical values and gamma in Montgomery
// form, so no conversions; no LDS.  The quotient of f is the kernels above on f, and the y_k = p_k(z) are their "totals" role over
// G K pairs, pair g K + k taking z_g through kzg_points_kernel's index divisor.  The verifier's L = sum_k gamma^k C_k - y_f G1 + z W
// is K + 2 terms: kzg_fold_points_kernel, one wave per workgroup for xyzz_mul_short's registers, multiplies a chunk of 64 terms
// side by side (gamma^k by square-and-multiply in the thread; y_f by Horner in the thread of the term -y_f G1) and adds them in a
// tree of xyzz_add through LDS, so a group costs one multiplication and a tree whatever K is.  Every chunk leaves a partial sum and
// what it found wrong (a scalar at or above r, a refused point); kzg_fold_emit_kernel, one thread per group, adds the partials and
// goes on as kzg_prepare_kernel does.  kzg_fold_sum_kernel ends the handle-free aid (sum_k gamma^k C_k alone).
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage for gfx950; every kernel: 0 bytes of scratch, no AGPRs; VGPRs, LDS per
// workgroup, waves / SIMD):
//   kzg_tile_kernel<256, totals> 55, 8 320 B, 8       kzg_tile_kernel<256, apply> 96, 8 320 B, 5
//   kzg_tile_kernel<1024, totals> 70, 36 992 B, 4     kzg_tile_kernel<1024, apply> 132, 36 992 B, 3
//   kzg_points_kernel 48, none, 8      kzg_prepare_kernel 212, none, 2      kzg_compare_kernel 71, none, 7
//   kzg_fold_kernel 56, none, 8        kzg_fold_points_kernel<check> 161, 8 192 B, 3      kzg_fold_points_kernel<aid> 176, 8 192 B, 2
//   kzg_fold_emit_kernel 127, none, 4  kzg_fold_sum_kernel 128, none, 4
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/graph_witness_groth16_verify.h"
#include "../../include/graph_witness_kzg.h"
#include "bn254_points_gfx950.hpp"
#include "groth16_internal.hpp"
#include "hip_util.hpp"
#include "kzg_internal.hpp"

using namespace cwc_r1cs;
using namespace cwc_g16;
using cwc::Fr;

namespace {

constexpr uint32_t THREADS = 256, WAVE = 64, WAVES = THREADS / WAVE;

__device__ __forceinline__ Fr shfl_down_fr(const Fr& x, uint32_t delta) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = __shfl_down(x.v[i], delta, WAVE);
    return r;
}

// w mod r for any w < 2^256 (rare: (w R) / R through two products)
__device__ __forceinline__ Fr reduce_any(Fr w) {
    if (!cwc::u256_lt(w, cwc::fr_p())) w = cwc::fr_mul(cwc::fr_mul(w, cwc::fr_r2()), Fr{{1, 0, 0, 0, 0, 0, 0, 0}});
    return w;
}

// zs [..][32] canonical, any value; pair i of the K of this launch takes z = zs[(first + i) / div] (div > 1: the polynomials of a
// group share the group's point; first < div: how far into its group the launch's first pair lies) -> out[l K + i] = z^(TILE^l) in Montgomery form, l < levels
__global__ __launch_bounds__(THREADS) void kzg_points_kernel(const uint8_t* __restrict__ zs, uint32_t first, uint32_t div, uint32_t K, uint32_t levels,
                                                             uint32_t log_tile, Fr* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    Fr z = cwc::fr_mul(*reinterpret_cast<const Fr*>(zs + (size_t)((first + i) / div) * 32), cwc::fr_r2());  // (any first operand below 2^256)
    out[i] = z;
    for (uint32_t l = 1; l < levels; ++l) {
        for (uint32_t b = 0; b < log_tile; ++b) z = cwc::fr_sqr(z);
        out[(size_t)l * K + i] = z;
    }
}

// The LDS image of a tile in 16-byte units: element e at unit(e) and unit(e) + 1.
template <uint32_t TILE>
struct Shape {
    static constexpr uint32_t RUN = TILE / THREADS;
    static constexpr uint32_t UNITS = 2 * TILE + (RUN > 1 ? THREADS : 0);
    static __device__ __forceinline__ uint32_t unit(uint32_t e) { return 2 * e + (RUN > 1 ? e / RUN : 0); }
};

// Tile blockIdx.x of pair blockIdx.y of the level whose n elements per pair lie at `in` (in_stride bytes from pair to pair) and
// whose point is zs[pair].  APPLY = false: totals[pair totals_stride + tile] = B_tile.  APPLY = true: with K_tile =
// carry[pair carry_stride + tile] (0 for the last tile and without `carry`), s_0 -> y_out[pair] (unless null) and s_i -> element
// i - 1 of q_out (q_stride bytes from pair to pair; unless null).
template <uint32_t TILE, bool APPLY>
__global__ __launch_bounds__(THREADS) void kzg_tile_kernel(const uint8_t* __restrict__ in, size_t in_stride, uint32_t n, uint32_t reduce,
                                                           const Fr* __restrict__ zs, const Fr* __restrict__ carry, uint32_t carry_stride,
                                                           Fr* __restrict__ totals, uint32_t totals_stride, uint8_t* __restrict__ y_out,
                                                           uint8_t* __restrict__ q_out, size_t q_stride) {
    using S = Shape<TILE>;
    constexpr uint32_t RUN = S::RUN;
    static_assert(TILE % THREADS == 0 && (RUN & (RUN - 1)) == 0, "a run per thread, a power of two long");
    __shared__ uint4 stage[S::UNITS];
    __shared__ Fr wave_sum[WAVES];
    const uint32_t tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, tile = blockIdx.x, pair = blockIdx.y;
    const uint32_t first = tile * TILE, avail = min(TILE, n - first);  // (the grid has ceil(n / TILE) tiles: first < n)
    const Fr z = zs[pair];

    const uint4* src = reinterpret_cast<const uint4*>(in + (size_t)pair * in_stride) + (size_t)first * 2;
#pragma unroll
    for (uint32_t k = 0; k < 2 * RUN; ++k) {
        const uint32_t j = tid + k * THREADS, e = j >> 1;
        stage[S::unit(e) + (j & 1u)] = e < avail ? src[j] : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    Fr c[RUN];
#pragma unroll
    for (uint32_t r = 0; r < RUN; ++r) {
        const uint4 lo = stage[S::unit(tid * RUN + r)], hi = stage[S::unit(tid * RUN + r) + 1];
        c[r] = Fr{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
        if (reduce) c[r] = reduce_any(c[r]);
    }

    Fr x = c[RUN - 1];
#pragma unroll
    for (int r = (int)RUN - 2; r >= 0; --r) x = cwc::fr_add(c[r], cwc::fr_mul(x, z));

    Fr m = z;  // z^RUN, then z^(RUN 2^d)
#pragma unroll
    for (uint32_t b = 1; b < RUN; b <<= 1) m = cwc::fr_sqr(m);
    Fr p = cwc::fr_one();  // z^(RUN (64 - lane)) in the end (apply)
    const uint32_t up = WAVE - lane;
#pragma unroll
    for (uint32_t d = 0; d < 6; ++d) {
        const Fr t = cwc::fr_add(x, cwc::fr_mul(shfl_down_fr(x, 1u << d), m));
        x = cwc::u256_select(lane + (1u << d) < WAVE, t, x);
        if constexpr (APPLY) p = cwc::u256_select(((up >> d) & 1u) != 0, cwc::fr_mul(p, m), p);
        m = cwc::fr_sqr(m);
    }
    // m = z^(64 RUN): a wave's span
    if (lane == 0) wave_sum[wave] = x;
    __syncthreads();  // (and every thread has read its run: the stage is free)
    Fr k = cwc::fr_zero();
    if constexpr (APPLY)
        if (carry && tile + 1 < gridDim.x) k = carry[(size_t)pair * carry_stride + tile];
    for (uint32_t w = WAVES - 1; w > wave; --w) k = cwc::fr_add(wave_sum[w], cwc::fr_mul(k, m));

    if constexpr (!APPLY) {
        if (tid == 0) totals[(size_t)pair * totals_stride + tile] = cwc::fr_add(x, cwc::fr_mul(k, m));
    } else {
        p = cwc::u256_select((up >> 6) != 0, cwc::fr_mul(p, m), p);
        x = cwc::fr_add(x, cwc::fr_mul(k, p));  // the suffix sum at the run's first coefficient, everything above included
        Fr s = shfl_down_fr(x, 1);
        s = cwc::u256_select(lane == WAVE - 1, k, s);  // the one at the next run's
#pragma unroll
        for (int r = (int)RUN - 1; r >= 0; --r) {
            s = cwc::fr_add(c[r], cwc::fr_mul(s, z));
            const uint32_t u = S::unit(tid * RUN + (uint32_t)r);
            stage[u] = make_uint4(s.v[0], s.v[1], s.v[2], s.v[3]);
            stage[u + 1] = make_uint4(s.v[4], s.v[5], s.v[6], s.v[7]);
        }
        __syncthreads();
        uint4* q = q_out ? reinterpret_cast<uint4*>(q_out + (size_t)pair * q_stride) : nullptr;
        uint4* y = y_out ? reinterpret_cast<uint4*>(y_out + (size_t)pair * 32) : nullptr;
#pragma unroll
        for (uint32_t kk = 0; kk < 2 * RUN; ++kk) {
            const uint32_t j = tid + kk * THREADS, e = j >> 1;
            if (e >= avail) continue;
            const uint4 v = stage[S::unit(e) + (j & 1u)];
            const size_t i = (size_t)first + e;
            if (i == 0) {
                if (y) y[j & 1u] = v;
            } else if (q) {
                q[(i - 1) * 2 + (j & 1u)] = v;
            }
        }
    }
}

template <uint32_t TILE>
void launch_level(bool apply, uint32_t blocks, uint32_t pairs, hipStream_t s, const uint8_t* in, size_t in_stride, uint32_t n, bool reduce, const Fr* zs,
                  const Fr* carry, uint32_t carry_stride, Fr* totals, uint32_t totals_stride, uint8_t* y_out, uint8_t* q_out, size_t q_stride) {
    if (apply)
        hipLaunchKernelGGL((kzg_tile_kernel<TILE, true>), dim3(blocks, pairs), dim3(THREADS), 0, s, in, in_stride, n, reduce ? 1u : 0u, zs, carry, carry_stride,
                           totals, totals_stride, y_out, q_out, q_stride);
    else
        hipLaunchKernelGGL((kzg_tile_kernel<TILE, false>), dim3(blocks, pairs), dim3(THREADS), 0, s, in, in_stride, n, reduce ? 1u : 0u, zs, carry, carry_stride,
                           totals, totals_stride, y_out, q_out, q_stride);
}

constexpr uint32_t MAX_LEVELS = 4;  // 256^4 = 2^32 coefficients

// The levels of one call: level l has n[l] elements per pair in blocks[l] tiles; its totals are level l + 1's elements.
struct Levels {
    uint32_t count = 0, n[MAX_LEVELS] = {}, blocks[MAX_LEVELS] = {};
    size_t o_z = 0, o_tot[MAX_LEVELS] = {}, o_carry[MAX_LEVELS] = {}, bytes = 0;  // o_tot[l], o_carry[l]: [pairs][blocks[l]] Fr
    Levels(uint64_t pairs, uint64_t N, uint32_t tile) {
        for (uint64_t len = N; count < MAX_LEVELS; len = blocks[count - 1]) {
            n[count] = (uint32_t)len;
            blocks[count] = (uint32_t)((len + tile - 1) / tile);
            if (blocks[count++] <= 1) break;
        }
        Carve cw;
        o_z = cw.take(pairs * count * 32);
        for (uint32_t l = 0; l + 1 < count; ++l) {
            o_tot[l] = cw.take(pairs * blocks[l] * 32);
            o_carry[l] = cw.take(pairs * blocks[l] * 32);
        }
        bytes = cw.o;
    }
};

uint32_t log2_of(uint32_t tile) { return 31u - (uint32_t)__builtin_clz(tile); }

// Opening i's status and its pairing inputs (L, G2), (W, tauG2); the generators for an opening that is decided already
__device__ __forceinline__ void put_pairing_inputs(uint32_t i, uint32_t st, const A1& l, const A1& w, const uint8_t* __restrict__ tau_g2, uint8_t* __restrict__ g1,
                                                   uint8_t* __restrict__ g2, uint32_t* __restrict__ status) {
    status[i] = st;
    uint8_t* o1 = g1 + (size_t)i * 2 * G1_BYTES;
    uint8_t* o2 = g2 + (size_t)i * 2 * G2_BYTES;
    const A2 gen2 = g2_generator();
    put_coords<G2>(o2, gen2.x, gen2.y, true);
    if (st == cwc_kzg::PENDING) {
        put_coords<G1>(o1, l.x, l.y, true);
        put_coords<G1>(o1 + G1_BYTES, w.x, w.y, true);
#pragma unroll
        for (int k = 0; k < 8; ++k) reinterpret_cast<uint4*>(o2 + G2_BYTES)[k] = reinterpret_cast<const uint4*>(tau_g2)[k];
    } else {
        const A1 gen = g1_generator();
        put_coords<G1>(o1, gen.x, gen.y, true);
        put_coords<G1>(o1 + G1_BYTES, gen.x, gen.y, true);
        put_coords<G2>(o2 + G2_BYTES, gen2.x, gen2.y, true);
    }
}

__global__ __launch_bounds__(WAVE) void kzg_prepare_kernel(const uint8_t* __restrict__ cs, const uint8_t* __restrict__ zs, const uint8_t* __restrict__ ys,
                                                           const uint8_t* __restrict__ ws, uint32_t K, const uint8_t* __restrict__ tau_g2,
                                                           uint8_t* __restrict__ g1, uint8_t* __restrict__ g2, uint32_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    const Fr y = *reinterpret_cast<const Fr*>(ys + (size_t)i * 32), z = *reinterpret_cast<const Fr*>(zs + (size_t)i * 32);
    A1 c, w;
    const PointFault fc = get_point<G1>(cs + (size_t)i * G1_BYTES, true, c), fw = get_point<G1>(ws + (size_t)i * G1_BYTES, true, w);
    uint32_t st = cwc_kzg::PENDING;
    A1 l = g1_generator();
    if (!cwc::both(cwc::u256_lt(y, cwc::fr_p()), cwc::u256_lt(z, cwc::fr_p()))) {
        st = GWB_KZG_SCALAR;
    } else if (fc != PointFault::NONE || fw != PointFault::NONE) {
        st = GWB_KZG_POINT;
    } else {
        const A1 gen = g1_generator();
        const P1 yg = xyzz_mul_short(P1{gen.x, gen.y, G1::one(), G1::one()}, y), zw = xyzz_mul_short(from_affine(w), z);
        l = xyzz_to_affine(xyzz_add(from_affine(c), xyzz_add(xyzz_neg(yg), zw)));
        const bool l_inf = affine_is_inf(l), w_inf = affine_is_inf(w);
        if (l_inf || w_inf) st = l_inf && w_inf ? GWB_KZG_VALID : GWB_KZG_EQUATION;
    }
    put_pairing_inputs(i, st, l, w, tau_g2, g1, g2, status);
}

__global__ __launch_bounds__(THREADS) void kzg_compare_kernel(const uint8_t* __restrict__ gt, uint32_t K, uint32_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K || status[i] != cwc_kzg::PENDING) return;
    const uint4* a = reinterpret_cast<const uint4*>(gt + (size_t)i * 2 * GWB_GT_BYTES);
    const uint4* b = a + GWB_GT_BYTES / 16;
    uint32_t diff = 0;
    for (uint32_t k = 0; k < GWB_GT_BYTES / 16; ++k) diff |= (a[k].x ^ b[k].x) | (a[k].y ^ b[k].y) | (a[k].z ^ b[k].z) | (a[k].w ^ b[k].w);
    status[i] = diff ? GWB_KZG_EQUATION : GWB_KZG_VALID;
}

// -- folded openings ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Fr load_fr(const uint4* __restrict__ p) {
    const uint4 lo = p[0], hi = p[1];
    return Fr{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
}

// polys [G][K][N][32], gammas [G][32], any values -> out [G][N][32] = sum_k gamma^k p_k, canonical.  Group blockIdx.y, one thread
// per coefficient index: Horner in gamma from the last polynomial down.
__global__ __launch_bounds__(THREADS) void kzg_fold_kernel(const uint8_t* __restrict__ polys, const uint8_t* __restrict__ gammas, uint32_t K, uint32_t N,
                                                           uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x, g = blockIdx.y;
    if (i >= N) return;
    const Fr gm = cwc::fr_mul(*reinterpret_cast<const Fr*>(gammas + (size_t)g * 32), cwc::fr_r2());  // (any first operand below 2^256)
    const size_t step = (size_t)N * 2;
    const uint4* src = reinterpret_cast<const uint4*>(polys) + ((size_t)g * K * N + i) * 2;
    Fr acc = reduce_any(load_fr(src + (size_t)(K - 1) * step));
    for (uint32_t k = K - 1; k-- > 0;) acc = cwc::fr_add(reduce_any(load_fr(src + (size_t)k * step)), cwc::fr_mul(acc, gm));
    uint4* dst = reinterpret_cast<uint4*>(out) + ((size_t)g * N + i) * 2;
    dst[0] = make_uint4(acc.v[0], acc.v[1], acc.v[2], acc.v[3]);
    dst[1] = make_uint4(acc.v[4], acc.v[5], acc.v[6], acc.v[7]);
}

constexpr uint32_t FOLD_SCALAR = 1u, FOLD_POINT = 2u;  // what a chunk of a group's terms found wrong

// base^e, Montgomery form in and out
__device__ __forceinline__ Fr fr_pow_u32(Fr base, uint32_t e) {
    Fr r = cwc::fr_one();
    for (; e; e >>= 1) {
        if (e & 1u) r = cwc::fr_mul(r, base);
        base = cwc::fr_sqr(base);
    }
    return r;
}

// The linear combination of a group's points, one term per thread and one wave per workgroup: workgroup (chunk, group) multiplies
// the terms chunk * 64 .. + 63 side by side and adds them in a tree through LDS; the sum goes to partials[group chunks + chunk]
// (XYZZ, Montgomery form) and what the chunk found wrong to flags[..].  Term k < K is gamma^k C_k.  CHECK (the verifier) adds
// term K = -y_f G1, y_f = sum_k gamma^k y_k by Horner in that one thread, and term K + 1 = z W, and flags a gamma, z or y_k at or
// above r; without it gamma is reduced.  A point that get_point refuses is flagged and left out.
template <bool CHECK>
__global__ __launch_bounds__(WAVE) void kzg_fold_points_kernel(const uint8_t* __restrict__ cs, const uint8_t* __restrict__ gammas, const uint8_t* __restrict__ zs,
                                                               const uint8_t* __restrict__ ys, const uint8_t* __restrict__ ws, uint32_t K,
                                                               P1* __restrict__ partials, uint32_t* __restrict__ flags) {
    __shared__ P1 tree[WAVE];
    const uint32_t lane = threadIdx.x, chunk = blockIdx.x, chunks = gridDim.x, g = blockIdx.y, t = chunk * WAVE + lane;
    const Fr gamma = *reinterpret_cast<const Fr*>(gammas + (size_t)g * 32);
    const Fr gm = cwc::fr_mul(gamma, cwc::fr_r2());  // (any first operand below 2^256)
    uint32_t fl = CHECK && !cwc::u256_lt(gamma, cwc::fr_p()) ? FOLD_SCALAR : 0u;
    A1 a = g1_generator();
    Fr k = cwc::fr_zero();
    bool live = false;
    if (t < K) {
        live = get_point<G1>(cs + ((size_t)g * K + t) * G1_BYTES, true, a) == PointFault::NONE;
        if (live)
            k = cwc::fr_from_mont(fr_pow_u32(gm, t));
        else
            fl |= FOLD_POINT;
    } else if (CHECK && t == K) {
        const uint8_t* y = ys + (size_t)g * K * 32;
        for (uint32_t j = K; j-- > 0;) {
            const Fr yj = *reinterpret_cast<const Fr*>(y + (size_t)j * 32);
            if (!cwc::u256_lt(yj, cwc::fr_p())) fl |= FOLD_SCALAR;
            k = cwc::fr_add(yj, cwc::fr_mul(k, gm));
        }
        a.y = G1::neg(a.y);
        live = true;
    } else if (CHECK && t == K + 1) {
        k = *reinterpret_cast<const Fr*>(zs + (size_t)g * 32);
        if (!cwc::u256_lt(k, cwc::fr_p())) fl |= FOLD_SCALAR;
        live = get_point<G1>(ws + (size_t)g * G1_BYTES, true, a) == PointFault::NONE;
        if (!live) fl |= FOLD_POINT;
    }
    P1 term = xyzz_inf<G1>();
    if (live) term = xyzz_mul_short(from_affine(a), k);
    tree[lane] = term;
    for (uint32_t s = WAVE / 2; s; s >>= 1) {
        __syncthreads();
        if (lane < s) {  // (reads [s, 2s), writes [0, s))
            term = xyzz_add(term, tree[lane + s]);
            tree[lane] = term;
        }
    }
    const uint32_t all = (__any(fl & FOLD_SCALAR) ? FOLD_SCALAR : 0u) | (__any(fl & FOLD_POINT) ? FOLD_POINT : 0u);
    if (lane == 0) {
        partials[(size_t)g * chunks + chunk] = term;
        flags[(size_t)g * chunks + chunk] = all;
    }
}

// the sum of a group's partial sums, and everything its chunks found wrong
__device__ __forceinline__ P1 sum_partials(const P1* __restrict__ p, const uint32_t* __restrict__ f, uint32_t chunks, uint32_t& fl) {
    P1 s = p[0];
    fl = f[0];
    for (uint32_t c = 1; c < chunks; ++c) {
        s = xyzz_add(s, p[c]);
        fl |= f[c];
    }
    return s;
}

// The folded check's kzg_prepare_kernel, one thread per group: L is the sum of the group's partials, and the status and the pairing
// inputs follow as there.
__global__ __launch_bounds__(WAVE) void kzg_fold_emit_kernel(const P1* __restrict__ partials, const uint32_t* __restrict__ flags, uint32_t chunks,
                                                             const uint8_t* __restrict__ ws, uint32_t G, const uint8_t* __restrict__ tau_g2,
                                                             uint8_t* __restrict__ g1, uint8_t* __restrict__ g2, uint32_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G) return;
    uint32_t fl;
    const P1 sum = sum_partials(partials + (size_t)i * chunks, flags + (size_t)i * chunks, chunks, fl);
    A1 w, l = g1_generator();
    (void)get_point<G1>(ws + (size_t)i * G1_BYTES, true, w);  // (a W that fails is flagged already)
    uint32_t st = cwc_kzg::PENDING;
    if (fl & FOLD_SCALAR) {
        st = GWB_KZG_SCALAR;
    } else if (fl & FOLD_POINT) {
        st = GWB_KZG_POINT;
    } else {
        l = xyzz_to_affine(sum);
        const bool l_inf = affine_is_inf(l), w_inf = affine_is_inf(w);
        if (l_inf || w_inf) st = l_inf && w_inf ? GWB_KZG_VALID : GWB_KZG_EQUATION;
    }
    put_pairing_inputs(i, st, l, w, tau_g2, g1, g2, status);
}

// The aid's end: out[i] = the sum of group i's partials, 64 canonical bytes; *fault = the lowest group with a refused point
__global__ __launch_bounds__(WAVE) void kzg_fold_sum_kernel(const P1* __restrict__ partials, const uint32_t* __restrict__ flags, uint32_t chunks, uint32_t G,
                                                            uint8_t* __restrict__ out, uint32_t* __restrict__ fault) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G) return;
    uint32_t fl;
    const A1 sum = xyzz_to_affine(sum_partials(partials + (size_t)i * chunks, flags + (size_t)i * chunks, chunks, fl));
    put_coords<G1>(out + (size_t)i * G1_BYTES, sum.x, sum.y, true);
    if (fl & FOLD_POINT) atomicMin(fault, i);
}

}  // namespace

namespace cwc_kzg {

size_t eval_quotient_ws(uint64_t K, uint64_t N, uint32_t tile) { return Levels(std::min<uint64_t>(K, MAX_PAIRS_PER_LAUNCH), N, tile).bytes; }

bool enqueue_eval_quotient(const uint8_t* d_polys, const uint8_t* d_zs, uint32_t z_div, uint64_t K, uint32_t N, uint32_t tile, uint8_t* d_ys, uint8_t* d_qs,
                           uint8_t* d_ws, hipStream_t s, std::string& err) {
    const uint64_t piece = std::min<uint64_t>(K, MAX_PAIRS_PER_LAUNCH);
    const Levels lv(piece, N, tile);
    const auto launch = tile == TILE_SMALL ? launch_level<TILE_SMALL> : launch_level<TILE_PRODUCTION>;
    Fr* zs = (Fr*)(d_ws + lv.o_z);
    const size_t q_stride = (size_t)(N - 1) * 32;
    for (uint64_t at = 0; at < K; at += piece) {
        const uint32_t pairs = (uint32_t)std::min<uint64_t>(piece, K - at);
        const uint8_t* polys = d_polys + at * N * 32;
        // (the piece's first point by a 64-bit offset; what is left of `at` is below z_div, so first + i stays 32-bit in the kernel)
        hipLaunchKernelGGL(kzg_points_kernel, dim3(blocks_for(pairs, THREADS)), dim3(THREADS), 0, s, d_zs + at / z_div * 32, (uint32_t)(at % z_div), z_div, pairs,
                           lv.count, log2_of(tile), zs);
        // level l's elements: the coefficients, or the totals of the level below
        auto in_of = [&](uint32_t l) { return l ? d_ws + lv.o_tot[l - 1] : polys; };
        auto stride_of = [&](uint32_t l) { return l ? (size_t)lv.blocks[l - 1] * 32 : (size_t)N * 32; };
        for (uint32_t l = 0; l + 1 < lv.count; ++l)
            launch(false, lv.blocks[l], pairs, s, in_of(l), stride_of(l), lv.n[l], l == 0, zs + (size_t)l * pairs, nullptr, 0, (Fr*)(d_ws + lv.o_tot[l]), lv.blocks[l],
                   nullptr, nullptr, 0);
        for (uint32_t l = lv.count; l-- > 0;) {
            const bool top = l + 1 == lv.count;
            if (!d_qs && !top) break;  // an evaluation alone is the top level's y
            uint8_t* q_out = !d_qs ? nullptr : l ? d_ws + lv.o_carry[l - 1] : d_qs + at * q_stride;
            uint8_t* y_out = l == 0 || !d_qs ? d_ys + at * 32 : nullptr;
            launch(true, lv.blocks[l], pairs, s, in_of(l), stride_of(l), lv.n[l], l == 0, zs + (size_t)l * pairs, top ? nullptr : (const Fr*)(d_ws + lv.o_carry[l]),
                   lv.blocks[l], nullptr, 0, y_out, q_out, l ? (size_t)lv.blocks[l - 1] * 32 : q_stride);
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) err = hip_err("launching the evaluate-and-quotient kernels", e);
    return e == hipSuccess;
}

bool enqueue_prepare(const uint8_t* d_c, const uint8_t* d_z, const uint8_t* d_y, const uint8_t* d_w, uint32_t K, const uint8_t* d_tau_g2, uint8_t* d_g1,
                     uint8_t* d_g2, uint32_t* d_status, hipStream_t s, std::string& err) {
    hipLaunchKernelGGL(kzg_prepare_kernel, dim3(blocks_for(K, WAVE)), dim3(WAVE), 0, s, d_c, d_z, d_y, d_w, K, d_tau_g2, d_g1, d_g2, d_status);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) err = hip_err("launching the opening check's preparation", e);
    return e == hipSuccess;
}

bool enqueue_fold(const uint8_t* d_polys, const uint8_t* d_gammas, uint64_t G, uint32_t K, uint32_t N, uint8_t* d_out, hipStream_t s, std::string& err) {
    for (uint64_t at = 0; at < G; at += MAX_PAIRS_PER_LAUNCH) {
        const uint32_t groups = (uint32_t)std::min<uint64_t>(MAX_PAIRS_PER_LAUNCH, G - at);
        hipLaunchKernelGGL(kzg_fold_kernel, dim3(blocks_for(N, THREADS), groups), dim3(THREADS), 0, s, d_polys + at * K * N * 32, d_gammas + at * 32, K, N,
                           d_out + at * N * 32);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) err = hip_err("launching the fold kernel", e);
    return e == hipSuccess;
}

// chunks of 64 terms in a group's linear combination (K <= MAX_FOLD_PAIRS: K + 2 fits)
static uint32_t fold_chunks(uint32_t K, bool check) { return (uint32_t)(((uint64_t)K + (check ? 2 : 0) + WAVE - 1) / WAVE); }

size_t fold_points_ws(uint64_t G, uint32_t K, bool check) { return (size_t)(G * fold_chunks(K, check)) * FOLD_PARTIAL_BYTES; }

bool enqueue_fold_points(const uint8_t* d_c, const uint8_t* d_gammas, const uint8_t* d_z, const uint8_t* d_y, const uint8_t* d_w, uint64_t G, uint32_t K,
                         uint8_t* d_ws, hipStream_t s, std::string& err) {
    static_assert(sizeof(P1) + sizeof(uint32_t) <= FOLD_PARTIAL_BYTES, "a partial sum and its flags");
    const bool check = d_w != nullptr;
    const uint32_t chunks = fold_chunks(K, check);
    P1* partials = reinterpret_cast<P1*>(d_ws);
    uint32_t* flags = reinterpret_cast<uint32_t*>(d_ws + (size_t)(G * chunks) * sizeof(P1));
    for (uint64_t at = 0; at < G; at += MAX_PAIRS_PER_LAUNCH) {
        const dim3 grid(chunks, (uint32_t)std::min<uint64_t>(MAX_PAIRS_PER_LAUNCH, G - at));
        if (check)
            hipLaunchKernelGGL(kzg_fold_points_kernel<true>, grid, dim3(WAVE), 0, s, d_c + at * K * G1_BYTES, d_gammas + at * 32, d_z + at * 32, d_y + at * K * 32,
                               d_w + at * G1_BYTES, K, partials + at * chunks, flags + at * chunks);
        else
            hipLaunchKernelGGL(kzg_fold_points_kernel<false>, grid, dim3(WAVE), 0, s, d_c + at * K * G1_BYTES, d_gammas + at * 32, nullptr, nullptr, nullptr, K,
                               partials + at * chunks, flags + at * chunks);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) err = hip_err("launching the point fold", e);
    return e == hipSuccess;
}

bool enqueue_fold_emit(const uint8_t* d_ws, const uint8_t* d_w, uint32_t G, uint32_t K, const uint8_t* d_tau_g2, uint8_t* d_g1, uint8_t* d_g2, uint32_t* d_status,
                       hipStream_t s, std::string& err) {
    const uint32_t chunks = fold_chunks(K, true);
    hipLaunchKernelGGL(kzg_fold_emit_kernel, dim3(blocks_for(G, WAVE)), dim3(WAVE), 0, s, reinterpret_cast<const P1*>(d_ws),
                       reinterpret_cast<const uint32_t*>(d_ws + (size_t)G * chunks * sizeof(P1)), chunks, d_w, G, d_tau_g2, d_g1, d_g2, d_status);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) err = hip_err("launching the folded check's preparation", e);
    return e == hipSuccess;
}

bool enqueue_fold_sum(const uint8_t* d_ws, uint32_t G, uint32_t K, uint8_t* d_out, uint32_t* d_fault, hipStream_t s, std::string& err) {
    const uint32_t chunks = fold_chunks(K, false);
    hipLaunchKernelGGL(kzg_fold_sum_kernel, dim3(blocks_for(G, WAVE)), dim3(WAVE), 0, s, reinterpret_cast<const P1*>(d_ws),
                       reinterpret_cast<const uint32_t*>(d_ws + (size_t)G * chunks * sizeof(P1)), chunks, G, d_out, d_fault);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) err = hip_err("launching the point fold's sum", e);
    return e == hipSuccess;
}

bool enqueue_compare(const uint8_t* d_gt, uint32_t K, uint32_t* d_status, hipStream_t s, std::string& err) {
    hipLaunchKernelGGL(kzg_compare_kernel, dim3(blocks_for(K, THREADS)), dim3(THREADS), 0, s, d_gt, K, d_status);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) err = hip_err("launching the opening check's comparison", e);
    return e == hipSuccess;
}

}  // namespace cwc_kzg
