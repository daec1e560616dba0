// Groth16 prover on gfx950 (include/graph_witness_groth16.h has the definition): per witness row, the witness map h
// (qap.hip), five multi-scalar multiplications by Pippenger's method, and the proof assembly.
//
// Scalars.  A row's MSM scalars are its nVars wires followed by r and s, so r delta1 and s delta1 / s delta2 ride in the A,
// B1 and B2 MSMs (their bases get two more points: A: delta1, O; B1: O, delta1; B2: O, delta2); C takes the wires nPub+1 ..
// nVars-1 of the same list.  h has its own list.  Each canonical scalar (< r < 2^254) is split into nWin signed c-bit digits
// d in [-2^(c-1) + 1, 2^(c-1)] (a carry moves up; nWin = floor(254 / c) + 1 windows take the last one); a nonzero digit is
// an entry (key = (row, window, |d| - 1), value = scalar index | sign), a zero digit gets the sentinel key, which sorts last.
//
// One sort, four MSMs.  The entries of a sub-batch are radix-sorted by key once (rocprim), and that order drives the A, B1, C
// and B2 accumulations; h's entries are sorted once for H.
//
// Accumulation, skew-proof.  The sorted list is cut into chunks of K entries, one thread per chunk, adding its entries' bases
// run by run (mixed XYZZ additions).  A run that lies inside one chunk is its bucket's whole sum and is written to the bucket;
// a run that crosses the chunk's first or last boundary leaves a partial (at most two per chunk).  The partials, compacted
// (rocprim select) and still sorted by key, are the next level's list; levels repeat until the list fits one chunk.  A
// bucket holding most of the entries (digit 1 of window 0 for a witness of bits) is summed by many threads, and the work is
// the number of nonzero digits, whatever their distribution.
//
// Reduction.  One wave per (row, window): lane t sums buckets t L .. t L + L - 1 by running sums (sum of (b + 1) bucket_b),
// the lanes are combined in LDS, and lane 0 multiplies by 2^(c window) (doublings); a last kernel adds the windows of a row.
//
// Assembly.  pi_A = alpha1 + MSM_A, B1 = beta1 + MSM_B1, pi_B = beta2 + MSM_B2; three threads per row form s pi_A, r B1 and
// -(r s) delta1 by double-and-add, three more add up pi_C and convert pi_A, pi_B, pi_C to canonical affine bytes.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <stdlib.h>
#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bn254_points_gfx950.hpp"
#include "groth16_internal.hpp"
#include "hip_util.hpp"
#include "lincomb.hpp"

using namespace cwc_r1cs;
using namespace cwc_g16;
using cwc::Fr;

namespace {

constexpr uint32_t K = 32;           // entries per accumulation chunk
constexpr uint32_t THREADS = 256;
constexpr uint32_t RED_LANES = 64;   // bucket segments per window (one wave)
constexpr uint32_t SIGN = 0x80000000u;

struct Msm {
    uint32_t n_sc = 0, c = 0, n_win = 0, n_b = 0;  // scalars per row, window bits, windows, buckets per window
};

Msm msm_shape(uint64_t n_sc) {
    Msm m;
    m.n_sc = (uint32_t)n_sc;
    uint32_t lg = 0;
    while ((2ull << lg) <= n_sc) ++lg;
    m.c = std::min<uint32_t>(15, std::max<uint32_t>(7, lg > 3 ? lg - 3 : 0));
    m.n_win = 254 / m.c + 1;
    m.n_b = 1u << (m.c - 1);
    return m;
}

__device__ __forceinline__ uint32_t bits_at(const Fr& k, uint32_t pos, uint32_t c) {  // c <= 16, pos < 256
    const uint32_t w = pos >> 5, s = pos & 31u;
    uint32_t lo = 0, hi = 0;  // k.v[w], k.v[w + 1] by selects (a dynamic index would put k on the stack)
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
        lo = i == w ? k.v[i] : lo;
        hi = i == w + 1 ? k.v[i] : hi;
    }
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    return (uint32_t)(v >> s) & ((1u << c) - 1u);
}

// the entries of every (row, scalar): scalar i < n_src from rows (stride n_stride elements, form), then r and s from rs
__global__ __launch_bounds__(THREADS) void digits_kernel(const uint8_t* __restrict__ src, uint32_t n_stride, uint32_t n_src, uint32_t montgomery,
                                                         const Fr* __restrict__ rs, uint32_t rows, Msm m, uint32_t sentinel,
                                                         uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint64_t total = (uint64_t)rows * m.n_sc;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t row = (uint32_t)(t / m.n_sc), i = (uint32_t)(t % m.n_sc);
        Fr k;
        if (i < n_src) {
            const Fr w = load_elem(src + (size_t)row * n_stride * 32, i);
            k = montgomery ? cwc::fr_from_mont(w) : reduce_any(w);
        } else {
            k = rs[2 * row + (i - n_src)];
        }
        uint32_t carry = 0;
        for (uint32_t win = 0; win < m.n_win; ++win) {
            const uint32_t pos = win * m.c;
            int32_t d = (int32_t)((pos < 256 ? bits_at(k, pos, m.c) : 0u) + carry);
            carry = 0;
            if (d > (int32_t)m.n_b) {
                d -= (int32_t)(2 * m.n_b);
                carry = 1;
            }
            const size_t o = ((size_t)row * m.n_win + win) * m.n_sc + i;
            if (d == 0) {
                keys[o] = sentinel;
                vals[o] = 0;
            } else {
                const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
                keys[o] = (row * m.n_win + win) * m.n_b + mag - 1;
                vals[o] = i | (d < 0 ? SIGN : 0u);
            }
        }
    }
}

template <class T>
__device__ __forceinline__ Affine<T> load_base(const Affine<T>* __restrict__ bases, uint32_t i) { return bases[i]; }

// One level of the chunked accumulation.  LEVEL0: entries (keys[j], vals[j]) name bases; scalar indices outside [lo, hi) are
// skipped, base = bases[index - lo].  Else: entry j is slot sel[j] of the previous level (in_keys, in_pts), count *d_count.
template <class T, bool LEVEL0>
__global__ __launch_bounds__(THREADS) void chunks_kernel(const uint32_t* __restrict__ in_keys, const uint32_t* __restrict__ vals,
                                                         const Xyzz<T>* __restrict__ in_pts, const uint32_t* __restrict__ sel,
                                                         const uint32_t* __restrict__ d_count, uint64_t m0, const Affine<T>* __restrict__ bases,
                                                         uint32_t lo, uint32_t hi, uint32_t sentinel, uint64_t n_chunks,
                                                         Xyzz<T>* __restrict__ buckets, uint32_t* __restrict__ out_keys,
                                                         Xyzz<T>* __restrict__ out_pts, uint32_t* __restrict__ out_flags) {
    const uint64_t ch = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= n_chunks) return;
    out_flags[2 * ch] = 0;
    out_flags[2 * ch + 1] = 0;
    const uint64_t m = LEVEL0 ? m0 : (uint64_t)*d_count;
    const uint64_t start = ch * K, end = start + K < m ? start + K : m;
    if (start >= m) return;
    auto key_at = [&](uint64_t j) -> uint32_t { return LEVEL0 ? in_keys[j] : in_keys[sel[j]]; };
    uint32_t key = key_at(start);
    if (key >= sentinel) return;
    const bool head_span = start > 0 && key_at(start - 1) == key;
    bool first_run = true;
    Xyzz<T> acc = xyzz_inf<T>();
    for (uint64_t j = start; j < end; ++j) {
        const uint32_t k = key_at(j);
        if (k != key) {
            if (first_run && head_span) {
                out_keys[2 * ch] = key;
                out_pts[2 * ch] = acc;
                out_flags[2 * ch] = 1;
            } else {
                buckets[key] = acc;
            }
            first_run = false;
            key = k;
            acc = xyzz_inf<T>();
            if (k >= sentinel) return;
        }
        if (LEVEL0) {
            const uint32_t v = vals[j], i = v & ~SIGN;
            if (i < lo || i >= hi) continue;
            Affine<T> b = load_base(bases, i - lo);
            if (affine_is_inf(b)) continue;
            if (v & SIGN) b.y = T::neg(b.y);
            acc = xyzz_add_affine(acc, b);
        } else {
            acc = xyzz_add(acc, in_pts[sel[j]]);
        }
    }
    const bool tail_span = end < m && key_at(end) == key;
    if (first_run && head_span) {
        out_keys[2 * ch] = key;
        out_pts[2 * ch] = acc;
        out_flags[2 * ch] = 1;
    } else if (tail_span) {
        out_keys[2 * ch + 1] = key;
        out_pts[2 * ch + 1] = acc;
        out_flags[2 * ch + 1] = 1;
    } else {
        buckets[key] = acc;
    }
}

template <class T>
__device__ __forceinline__ Xyzz<T> mul_small(const Xyzz<T>& p, uint32_t k) {  // k p, k < 2^16
    Xyzz<T> acc = xyzz_inf<T>();
    for (int b = 15; b >= 0; --b) {
        acc = xyzz_dbl(acc);
        if ((k >> b) & 1u) acc = xyzz_add(acc, p);
    }
    return acc;
}

// one wave per (row, window): sum_b (b + 1) bucket_b, times 2^(c window)
template <class T>
__global__ __launch_bounds__(RED_LANES) void reduce_kernel(const Xyzz<T>* __restrict__ buckets, Msm m, Xyzz<T>* __restrict__ win_out) {
    __shared__ Xyzz<T> part[RED_LANES];
    const uint32_t rw = blockIdx.x, win = rw % m.n_win, t = threadIdx.x;
    const uint32_t per = (m.n_b + RED_LANES - 1) / RED_LANES, b0 = t * per, b1 = b0 + per < m.n_b ? b0 + per : m.n_b;
    const Xyzz<T>* bk = buckets + (size_t)rw * m.n_b;
    Xyzz<T> run = xyzz_inf<T>(), acc = xyzz_inf<T>();
    for (uint32_t b = b1; b-- > b0;) {
        run = xyzz_add(run, bk[b]);
        acc = xyzz_add(acc, run);
    }
    if (b0 < b1) acc = xyzz_add(acc, mul_small(run, b0));
    part[t] = acc;
    __syncthreads();
    for (uint32_t s = RED_LANES / 2; s > 0; s >>= 1) {
        if (t < s) part[t] = xyzz_add(part[t], part[t + s]);
        __syncthreads();
    }
    if (t == 0) {
        Xyzz<T> x = part[0];
        for (uint32_t d = 0; d < win * m.c; ++d) x = xyzz_dbl(x);
        win_out[rw] = x;
    }
}

// out[row * stride] = sum of the row's windows
template <class T>
__global__ __launch_bounds__(THREADS) void windows_kernel(const Xyzz<T>* __restrict__ win_out, Msm m, uint32_t rows, Xyzz<T>* __restrict__ out,
                                                          uint32_t stride) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    Xyzz<T> acc = xyzz_inf<T>();
    for (uint32_t w = 0; w < m.n_win; ++w) acc = xyzz_add(acc, win_out[(size_t)row * m.n_win + w]);
    out[(size_t)row * stride] = acc;
}

struct Consts {
    Affine<G1> alpha1, beta1, delta1;
    Affine<G2> beta2;
};

// per row: G1 results [A, B1, C, H], G2 result B2; job 0: s pi_A, 1: r B1, 2: -(r s) delta1
__global__ __launch_bounds__(THREADS) void assemble_kernel(const P1* __restrict__ g1, const Fr* __restrict__ rs, Consts k, uint32_t rows,
                                                           P1* __restrict__ tmp) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * 3) return;
    const uint32_t row = t / 3, job = t % 3;
    const Fr r = rs[2 * row], s = rs[2 * row + 1];
    P1 x;
    if (job == 0) {
        x = xyzz_mul(xyzz_add(from_affine(k.alpha1), g1[4 * row]), s);
    } else if (job == 1) {
        x = xyzz_mul(xyzz_add(from_affine(k.beta1), g1[4 * row + 1]), r);
    } else {
        const Fr rsv = cwc::fr_mul(cwc::fr_to_mont(r), s);  // r s mod r, canonical
        x = xyzz_neg(xyzz_mul(from_affine(k.delta1), rsv));
    }
    tmp[t] = x;
}

// p -> canonical affine bytes
template <class T>
__device__ void put_affine(uint8_t* out, const Xyzz<T>& p) {
    const Affine<T> a = xyzz_to_affine(p);
    put_coords<T>(out, a.x, a.y, true);
}

// job 0: pi_A, 1: pi_B, 2: pi_C -> canonical affine bytes
__global__ __launch_bounds__(THREADS) void finish_kernel(const P1* __restrict__ g1, const P2* __restrict__ g2, const P1* __restrict__ tmp, Consts k,
                                                         uint32_t rows, uint8_t* __restrict__ proofs) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * 3) return;
    const uint32_t row = t / 3, job = t % 3;
    uint8_t* out = proofs + (size_t)row * GWB_GROTH16_PROOF_BYTES;
    if (job == 0) {
        put_affine<G1>(out, xyzz_add(from_affine(k.alpha1), g1[4 * row]));
    } else if (job == 1) {
        put_affine<G2>(out + 64, xyzz_add(from_affine(k.beta2), g2[row]));
    } else {
        P1 c = xyzz_add(g1[4 * row + 2], g1[4 * row + 3]);
        for (int i = 0; i < 3; ++i) c = xyzz_add(c, tmp[3 * row + i]);
        put_affine<G1>(out + 192, c);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------

uint64_t ws_cap() { return groth16_workspace_cap(); }

uint32_t bits_for(uint64_t x) {  // smallest b with 2^b > x
    uint32_t b = 0;
    while (b < 63 && (1ull << b) <= x) ++b;
    return b;
}

// The workspace of a sub-batch of `rows` rows, carved from one allocation.
struct Layout {
    Msm mw, mh;
    uint64_t m0 = 0;  // entries of the larger list
    uint32_t key_bits = 0;
    uint64_t slots0 = 0, slots1 = 0;  // slots of the even / odd accumulation levels
    size_t sort_tmp = 0, sel_tmp = 0;
    size_t off_h, off_keys[2], off_vals[2], off_buckets, off_slot_keys[2], off_slot_pts[2], off_flags[2], off_sel[2], off_count, off_win,
        off_g1, off_g2, off_tmp, off_sort_tmp, off_sel_tmp, total;
};

bool plan(const gwb_zkey* z, uint64_t rows, Layout& L, std::string& err) {
    const uint64_t nv = z->info.n_vars, n = z->info.domain_size;
    L.mw = msm_shape(nv + 2);
    L.mh = msm_shape(n);
    const uint64_t mw = rows * L.mw.n_win * L.mw.n_sc, mh = rows * L.mh.n_win * L.mh.n_sc;
    L.m0 = std::max(mw, mh);
    const uint64_t n_keys = std::max<uint64_t>(rows * L.mw.n_win * L.mw.n_b, rows * L.mh.n_win * L.mh.n_b);
    L.key_bits = bits_for(n_keys);  // keys < 2^key_bits; the sentinel is 2^key_bits
    if (L.key_bits > 31 || L.m0 > 0xffffffffull) {
        err = "groth16: sub-batch too large";
        return false;
    }
    const uint64_t ch0 = (L.m0 + K - 1) / K;
    L.slots0 = 2 * ch0;
    L.slots1 = 2 * ((L.slots0 + K - 1) / K);
    size_t s1 = 0, s2 = 0;
    rocprim::double_buffer<uint32_t> kb(nullptr, nullptr), vb(nullptr, nullptr);
    if (rocprim::radix_sort_pairs(nullptr, s1, kb, vb, (size_t)L.m0, 0, L.key_bits + 1) != hipSuccess ||
        rocprim::select(nullptr, s2, rocprim::counting_iterator<uint32_t>(0), (uint32_t*)nullptr, (uint32_t*)nullptr,
                        (uint32_t*)nullptr, (size_t)L.slots0) != hipSuccess) {
        err = "groth16: sizing the sort workspace failed";
        return false;
    }
    L.sort_tmp = s1;
    L.sel_tmp = s2;
    Carve cw;
    L.off_h = cw.take(rows * n * 32);
    for (int i = 0; i < 2; ++i) L.off_keys[i] = cw.take(L.m0 * 4);
    for (int i = 0; i < 2; ++i) L.off_vals[i] = cw.take(L.m0 * 4);
    L.off_buckets = cw.take(n_keys * sizeof(P2));
    for (int i = 0; i < 2; ++i) {
        const uint64_t s = i ? L.slots1 : L.slots0;
        L.off_slot_keys[i] = cw.take(s * 4);
        L.off_slot_pts[i] = cw.take(s * sizeof(P2));
        L.off_flags[i] = cw.take(s * 4);
        L.off_sel[i] = cw.take(s * 4);
    }
    L.off_count = cw.take(8);
    L.off_win = cw.take(rows * std::max(L.mw.n_win, L.mh.n_win) * sizeof(P2));
    L.off_g1 = cw.take(rows * 4 * sizeof(P1));
    L.off_g2 = cw.take(rows * sizeof(P2));
    L.off_tmp = cw.take(rows * 3 * sizeof(P1));
    L.off_sort_tmp = cw.take(L.sort_tmp);
    L.off_sel_tmp = cw.take(L.sel_tmp);
    L.total = cw.o;
    return true;
}

bool ensure_bases(gwb_zkey* z, std::string& err) {
    if (z->d_a) return true;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    std::vector<uint8_t> a(z->a), b1(z->b1), b2(z->b2);
    a.insert(a.end(), z->delta1, z->delta1 + G1_BYTES);
    a.insert(a.end(), G1_BYTES, 0);
    b1.insert(b1.end(), G1_BYTES, 0);
    b1.insert(b1.end(), z->delta1, z->delta1 + G1_BYTES);
    b2.insert(b2.end(), G2_BYTES, 0);
    b2.insert(b2.end(), z->delta2, z->delta2 + G2_BYTES);
    const std::vector<uint8_t>* src[5] = {&a, &b1, &b2, &z->c, &z->h};
    DeviceBuf* dst[5] = {&z->d_a, &z->d_b1, &z->d_b2, &z->d_c, &z->d_h};
    DeviceBuf up[5];  // the key gets all five or none
    for (int i = 0; i < 5 && e == hipSuccess; ++i) e = up[i].upload(src[i]->data(), src[i]->size());
    if (e != hipSuccess) {
        err = hip_err("uploading the zkey points", e);
        return false;
    }
    for (int i = 0; i < 5; ++i) *dst[i] = std::move(up[i]);
    z->device = dev;
    return true;
}

uint32_t grid_for(uint64_t threads, uint64_t cap = 1ull << 20) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((threads + THREADS - 1) / THREADS, cap));
}

struct Sub {
    uint8_t* ws;
    const Layout* L;
    uint64_t rows;
    hipStream_t s;
    template <class X>
    X* at(size_t off) const { return reinterpret_cast<X*>(ws + off); }
};

// entries of one scalar list, sorted; -> which of the two buffers holds the result
bool prep_sort(const Sub& S, const Msm& m, const uint8_t* src, uint32_t stride, uint32_t n_src, uint32_t mont, const Fr* rs, int& cur,
               std::string& err) {
    const Layout& L = *S.L;
    const uint32_t sentinel = 1u << L.key_bits;
    const uint64_t n_ent = S.rows * m.n_win * m.n_sc;
    hipLaunchKernelGGL(digits_kernel, dim3(grid_for(S.rows * m.n_sc, 16384)), dim3(THREADS), 0, S.s, src, stride, n_src, mont, rs,
                       (uint32_t)S.rows, m, sentinel, S.at<uint32_t>(L.off_keys[0]), S.at<uint32_t>(L.off_vals[0]));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        err = hip_err("launching the scalar digits", e);
        return false;
    }
    rocprim::double_buffer<uint32_t> kb(S.at<uint32_t>(L.off_keys[0]), S.at<uint32_t>(L.off_keys[1]));
    rocprim::double_buffer<uint32_t> vb(S.at<uint32_t>(L.off_vals[0]), S.at<uint32_t>(L.off_vals[1]));
    size_t tmp = L.sort_tmp;
    e = rocprim::radix_sort_pairs(S.at<void>(L.off_sort_tmp), tmp, kb, vb, (size_t)n_ent, 0, L.key_bits + 1, S.s);
    if (e != hipSuccess) {
        err = hip_err("sorting the scalar digits", e);
        return false;
    }
    cur = kb.current() == S.at<uint32_t>(L.off_keys[0]) ? 0 : 1;
    return true;
}

// one MSM over the sorted list `cur` of shape m: bases (index lo .. hi-1 of the scalar list) -> out[row * stride]
template <class T>
bool run_msm(const Sub& S, const Msm& m, int cur, const void* bases, uint32_t lo, uint32_t hi, Xyzz<T>* out, uint32_t stride, std::string& err) {
    const Layout& L = *S.L;
    const uint32_t sentinel = 1u << L.key_bits;
    const uint64_t n_ent = S.rows * m.n_win * m.n_sc, n_keys = S.rows * m.n_win * m.n_b;
    Xyzz<T>* buckets = S.at<Xyzz<T>>(L.off_buckets);
    hipError_t e = hipMemsetAsync(buckets, 0, n_keys * sizeof(Xyzz<T>), S.s);
    uint64_t bound = n_ent, n_ch = (bound + K - 1) / K;
    hipLaunchKernelGGL((chunks_kernel<T, true>), dim3(grid_for(n_ch)), dim3(THREADS), 0, S.s, S.at<uint32_t>(L.off_keys[cur]),
                       S.at<uint32_t>(L.off_vals[cur]), (const Xyzz<T>*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, n_ent,
                       (const Affine<T>*)bases, lo, hi, sentinel, n_ch, buckets, S.at<uint32_t>(L.off_slot_keys[0]),
                       S.at<Xyzz<T>>(L.off_slot_pts[0]), S.at<uint32_t>(L.off_flags[0]));
    if (e == hipSuccess) e = hipGetLastError();
    int lv = 0;
    while (e == hipSuccess && bound > K) {
        const uint64_t n_slots = 2 * n_ch;
        uint32_t* count = S.at<uint32_t>(L.off_count) + lv;
        size_t tmp = L.sel_tmp;
        e = rocprim::select(S.at<void>(L.off_sel_tmp), tmp, rocprim::counting_iterator<uint32_t>(0), S.at<uint32_t>(L.off_flags[lv]),
                            S.at<uint32_t>(L.off_sel[lv]), count, (size_t)n_slots, S.s);
        if (e != hipSuccess) break;
        bound = n_slots;
        n_ch = (bound + K - 1) / K;
        hipLaunchKernelGGL((chunks_kernel<T, false>), dim3(grid_for(n_ch)), dim3(THREADS), 0, S.s, S.at<uint32_t>(L.off_slot_keys[lv]),
                           (const uint32_t*)nullptr, S.at<Xyzz<T>>(L.off_slot_pts[lv]), S.at<uint32_t>(L.off_sel[lv]), count, (uint64_t)0,
                           (const Affine<T>*)nullptr, 0u, 0u, sentinel, n_ch, buckets, S.at<uint32_t>(L.off_slot_keys[lv ^ 1]),
                           S.at<Xyzz<T>>(L.off_slot_pts[lv ^ 1]), S.at<uint32_t>(L.off_flags[lv ^ 1]));
        e = hipGetLastError();
        lv ^= 1;
    }
    if (e == hipSuccess) {
        Xyzz<T>* win = S.at<Xyzz<T>>(L.off_win);
        hipLaunchKernelGGL(reduce_kernel<T>, dim3((uint32_t)(S.rows * m.n_win)), dim3(RED_LANES), 0, S.s, buckets, m, win);
        hipLaunchKernelGGL(windows_kernel<T>, dim3(grid_for(S.rows)), dim3(THREADS), 0, S.s, win, m, (uint32_t)S.rows, out, stride);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        err = hip_err("running an MSM", e);
        return false;
    }
    return true;
}

Consts consts_of(const gwb_zkey* z) {
    Consts k;
    memcpy(&k.alpha1, z->alpha1, G1_BYTES);
    memcpy(&k.beta1, z->beta1, G1_BYTES);
    memcpy(&k.delta1, z->delta1, G1_BYTES);
    memcpy(&k.beta2, z->beta2, G2_BYTES);
    return k;
}

void mark(gwb_zkey* z, int i, hipStream_t s) { z->events.record(i, s); }

bool enqueue_sub(gwb_zkey* z, gwb_r1cs* r, const Layout& L, const uint8_t* d_w, uint64_t rows, uint32_t form_in, const Fr* d_rs,
                 uint8_t* d_proofs, hipStream_t s, std::string& err) {
    Sub S{z->ws.as<uint8_t>(), &L, rows, s};
    const uint32_t nv = z->info.n_vars, n = z->info.domain_size, npub = z->info.n_public;
    const uint32_t mont = form_in == GWB_FORM_MONTGOMERY ? 1u : 0u;
    P1* g1 = S.at<P1>(L.off_g1);
    mark(z, 0, s);
    // the witness map: from the .r1cs, or with none given from the zkey's own section 4
    if (r ? !qap_enqueue(r, d_w, rows, form_in, S.at<void>(L.off_h), GWB_FORM_CANONICAL, s, err)
          : !qap_enqueue(z, d_w, rows, form_in, S.at<void>(L.off_h), GWB_FORM_CANONICAL, s, err))
        return false;
    mark(z, 1, s);
    int cur = 0;
    if (!prep_sort(S, L.mw, d_w, nv, nv, mont, d_rs, cur, err)) return false;
    mark(z, 2, s);
    if (!run_msm<G1>(S, L.mw, cur, z->d_a.as(), 0, nv + 2, g1 + 0, 4, err) || !run_msm<G1>(S, L.mw, cur, z->d_b1.as(), 0, nv + 2, g1 + 1, 4, err) ||
        !run_msm<G1>(S, L.mw, cur, z->d_c.as(), npub + 1, nv, g1 + 2, 4, err))
        return false;
    mark(z, 3, s);
    if (!run_msm<G2>(S, L.mw, cur, z->d_b2.as(), 0, nv + 2, S.at<P2>(L.off_g2), 1, err)) return false;
    mark(z, 4, s);
    if (!prep_sort(S, L.mh, S.at<uint8_t>(L.off_h), n, n, 0, nullptr, cur, err)) return false;
    mark(z, 5, s);
    if (!run_msm<G1>(S, L.mh, cur, z->d_h.as(), 0, n, g1 + 3, 4, err)) return false;
    mark(z, 6, s);
    const Consts k = consts_of(z);
    hipLaunchKernelGGL(assemble_kernel, dim3(grid_for(rows * 3)), dim3(THREADS), 0, s, g1, d_rs, k, (uint32_t)rows, S.at<P1>(L.off_tmp));
    hipLaunchKernelGGL(finish_kernel, dim3(grid_for(rows * 3)), dim3(THREADS), 0, s, g1, S.at<P2>(L.off_g2), S.at<P1>(L.off_tmp), k,
                       (uint32_t)rows, d_proofs);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        err = hip_err("launching the proof assembly", e);
        return false;
    }
    mark(z, 7, s);
    return true;
}

}  // namespace

namespace cwc_r1cs {
uint64_t groth16_workspace_cap() {  // CWC_GROTH16_WORKSPACE_MB, read once per process
    static const uint64_t cap = [] {
        const char* s = getenv("CWC_GROTH16_WORKSPACE_MB");
        const unsigned long long mb = s && *s ? strtoull(s, nullptr, 10) : 0ull;
        return (mb ? (uint64_t)mb : 4096ull) << 20;
    }();
    return cap;
}

bool draw_fr(Fr& x, std::string& err) {
    do {
        uint8_t* p = (uint8_t*)x.v;
        size_t got = 0;
        while (got < 32) {
            const ssize_t k = getrandom(p + got, 32 - got, 0);
            if (k < 0) {
                err = "groth16: getrandom failed";
                return false;
            }
            got += (size_t)k;
        }
        x.v[7] &= 0x3fffffffu;  // r < 2^254: draw 254 bits, keep those below r
    } while (!cwc::u256_lt(x, cwc::fr_p()));
    return true;
}
}  // namespace cwc_r1cs

namespace {

// rs for a batch: the caller's (each below r) or uniform draws from getrandom() by rejection
bool make_rs(const void* rs, size_t batch, std::vector<Fr>& out, std::string& err) {
    out.resize(batch * 2);
    if (rs) {
        memcpy(out.data(), rs, batch * 64);
        for (size_t i = 0; i < out.size(); ++i)
            if (!cwc::u256_lt(out[i], cwc::fr_p())) {
                err = "groth16: rs[" + std::to_string(i / 2) + "][" + std::to_string(i % 2) + "] is not below r";
                return false;
            }
        return true;
    }
    for (Fr& x : out)
        if (!draw_fr(x, err)) return false;
    return true;
}

// r == NULL: the zkey alone.  Its witness map is built here (host work), so what that refuses is refused before the device
// is touched.
bool check_pair(gwb_zkey* z, gwb_r1cs* r, size_t n_witness, size_t batch, std::string& err) {
    if (!r) {
        if (!zkey_coefs_build(z, err)) return false;
        if (n_witness != z->info.n_vars) {
            err = "groth16: the witness has " + std::to_string(n_witness) + " elements, the zkey nVars = " + std::to_string(z->info.n_vars);
            return false;
        }
        if (batch > 0xffffffffull) {
            err = "groth16: batch above 2^32 - 1";
            return false;
        }
        return true;
    }
    gwb_r1cs_qap_info_t qi;
    gw_status_t st{OK, nullptr};
    if (gwb_r1cs_qap_info(r, &qi, &st) != 0) {
        err = st.error_msg ? st.error_msg : "groth16: QAP domain";
        free(st.error_msg);
        return false;
    }
    const gwb_r1cs_info_t& ri = r->info;
    if (z->info.n_vars != ri.n_wires) {
        err = "groth16: zkey nVars " + std::to_string(z->info.n_vars) + " != r1cs nWires " + std::to_string(ri.n_wires);
        return false;
    }
    if (z->info.n_public != ri.n_pub_out + ri.n_pub_in) {
        err = "groth16: zkey nPublic " + std::to_string(z->info.n_public) + " != r1cs nPubOut + nPubIn " + std::to_string(ri.n_pub_out + ri.n_pub_in);
        return false;
    }
    if (z->info.domain_size != qi.domain_size) {
        err = "groth16: zkey domainSize " + std::to_string(z->info.domain_size) + " != r1cs QAP domain " + std::to_string(qi.domain_size);
        return false;
    }
    return check_args(r->sys, n_witness, batch, err);
}

bool enqueue_prove(gwb_zkey* z, gwb_r1cs* r, const void* d_w, size_t batch, uint32_t form_in, const std::vector<Fr>& rs, void* d_proofs,
                   hipStream_t s, std::string& err) {
    if (!ensure_bases(z, err)) return false;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev != z->device) {
        err = "groth16: the zkey's points live on device " + std::to_string(z->device) + ", the current device is " + std::to_string(dev);
        return false;
    }
    Layout one;
    if (!plan(z, 1, one, err)) return false;
    uint64_t sub = std::min<uint64_t>(batch, std::max<uint64_t>(1, ws_cap() / one.total));
    Layout L;
    while (true) {  // the per-row estimate from one row is close; shrink until the sub-batch fits
        if (!plan(z, sub, L, err)) return false;
        if (L.total + batch * 64 <= ws_cap() || sub == 1) break;
        sub = std::max<uint64_t>(1, sub * ws_cap() / (L.total + batch * 64 + 1));
    }
    const size_t rs_off = L.total;  // a multiple of 256
    if (!z->ws.ensure(rs_off + batch * 64, "allocating the prover workspace", err)) return false;
    Fr* d_rs = (Fr*)(z->ws.as<uint8_t>() + rs_off);
    // r, s go through a pinned buffer of the handle; the previous call's copy out of it is waited for first
    const hipError_t e = z->rs_stage.send(d_rs, rs.data(), batch * 64, s);
    if (e != hipSuccess) {
        err = hip_err("copying r, s", e);
        return false;
    }
    for (uint64_t s0 = 0; s0 < batch; s0 += sub) {
        const uint64_t rows = std::min<uint64_t>(sub, batch - s0);
        Layout Lr;
        if (!plan(z, rows, Lr, err)) return false;
        if (!enqueue_sub(z, r, Lr, (const uint8_t*)d_w + s0 * z->info.n_vars * 32, rows, form_in, d_rs + 2 * s0,
                         (uint8_t*)d_proofs + s0 * GWB_GROTH16_PROOF_BYTES, s, err))
            return false;
    }
    return true;
}

int prove_host(gwb_zkey* z, gwb_r1cs* r, const void* witness, size_t n_witness, size_t batch, const void* rs, void* proofs, gw_status_t* status) {
    std::string err;
    std::vector<Fr> rsv;
    if (!check_pair(z, r, n_witness, batch, err) || !make_rs(rs, batch, rsv, err)) return fail(status, err);
    if (batch == 0) {
        set_ok(status);
        return 0;
    }
    if (r && !ensure_device(r->sys, -1, err)) return fail(status, err);
    const size_t wbytes = batch * n_witness * 32, pbytes = batch * GWB_GROTH16_PROOF_BYTES;
    auto run = [&](unsigned char* const* d, hipStream_t s, std::string& err) {
        return enqueue_prove(z, r, d[0], batch, GWB_FORM_CANONICAL, rsv, d[1], s, err);
    };
    if (!run_staged({wbytes, pbytes}, {{witness, wbytes, 0, 0}}, {{proofs, pbytes, 1, 0}}, "staging the witness rows", "running the prover", run, err))
        return fail(status, err);
    set_ok(status);
    return 0;
}

}  // namespace

extern "C" {

void gwb_zkey_free(gwb_zkey_t* z) { delete z; }

int gwb_groth16_prove_batch_device(gwb_zkey_t* z, gwb_r1cs_t* r, const void* d_witness, size_t n_witness, size_t batch, uint32_t form_in,
                                   const void* rs, void* d_proofs, void* hip_stream, gw_status_t* status) {
    if (!z || (batch && (!d_witness || !d_proofs))) return fail(status, "gwb_groth16_prove_batch_device: NULL argument");
    if (form_in != GWB_FORM_CANONICAL && form_in != GWB_FORM_MONTGOMERY)
        return fail(status, "gwb_groth16_prove_batch_device: unknown form " + std::to_string(form_in));
    std::string err;
    std::vector<Fr> rsv;
    if (!check_pair(z, r, n_witness, batch, err) || !make_rs(rs, batch, rsv, err)) return fail(status, err);
    if (batch == 0) {
        set_ok(status);
        return 0;
    }
    if ((r && !ensure_device(r->sys, -1, err)) || !enqueue_prove(z, r, d_witness, batch, form_in, rsv, d_proofs, (hipStream_t)hip_stream, err))
        return fail(status, err);
    set_ok(status);
    return 0;
}

int gwb_groth16_prove_batch_host(gwb_zkey_t* z, gwb_r1cs_t* r, const void* witness, size_t n_witness, size_t batch, const void* rs, void* proofs,
                                 gw_status_t* status) {
    if (!z || (batch && (!witness || !proofs))) return fail(status, "gwb_groth16_prove_batch_host: NULL argument");
    return prove_host(z, r, witness, n_witness, batch, rs, proofs, status);
}

int gwb_groth16_prove_wtns(gwb_zkey_t* z, gwb_r1cs_t* r, const void* wtns, size_t len, const void* rs, void* proof, gw_status_t* status) {
    if (!z || !wtns || !proof) return fail(status, "gwb_groth16_prove_wtns: NULL argument");
    const uint8_t* values = nullptr;
    uint64_t n_wit = 0;
    std::string err;
    if (!parse_wtns(wtns, len, &values, &n_wit, err)) return fail(status, err);
    return prove_host(z, r, values, n_wit, 1, rs, proof, status);
}

int gwb_groth16_time_phases(gwb_zkey_t* z, int on) {
    if (!z) return 1;
    if (!on) z->events.off();
    return on && z->events.on() != hipSuccess ? 1 : 0;
}

int gwb_groth16_phase_ms(gwb_zkey_t* z, float* ms) {
    float d[7];
    if (!z || !ms || z->events.elapsed(d) != hipSuccess) return 1;
    ms[0] = d[0];         // witness map
    ms[1] = d[1] + d[4];  // scalar preparation and sort (w, h)
    ms[2] = d[2] + d[5];  // G1 MSMs (A, B1, C; H)
    ms[3] = d[3];         // G2 MSM
    ms[4] = d[6];         // assembly
    return 0;
}

}  // extern "C"
