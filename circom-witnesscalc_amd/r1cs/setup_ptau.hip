// Groth16 setup from a powers-of-tau file on gfx950 (include/graph_witness_groth16_ptau.h has the definition): no trapdoor, so no
// scalars to multiply generators by; every key point is a linear combination of the ceremony's points.  The host side that
// does not depend on where the points come from (column transpose and segments, section 4, conversion to affine, the zkey
// image) is setup.hip's (setup_internal.hpp); the `.ptau` itself is read by ptau.cc (ptau_internal.hpp).
//
// Loading.  The prefixes that are read are uploaded as stored; one thread per point checks the coordinate ranges and the curve
// equation and writes the point in XYZZ form (ZZ = ZZZ = 1, or 0 for infinity).  The first fault of an array goes to a flag
// word with atomicMin; the host turns it into the loader's message after the call's one synchronisation.
//
// Group inverse DFT.  Radix 2, decimation in time, in place on XYZZ points in global memory: the load writes point i to slot
// bitrev(i); stage s (half = 2^s) takes, for k < half and every group of 2 half slots, a = x[j], c = w_N^(-k N / (2 half))
// x[j + half] and writes a + c, a - c; the output is in natural order.  A twiddle is a 254-bit scalar, so a butterfly is one
// variable-base multiplication (fq_gfx950.hpp's xyzz_mul_short: double and add from the scalar's top word) and two additions; k = 0 has no
// multiplication (all of stage 0, and one butterfly per group after it).  The twiddles w_N^(-k), k < N / 2, are computed once
// per call into a table of canonical values.  While a stage has 64 or more groups, a wave's lanes take the same k in 64
// groups: the scalar is the same in every lane, so the wave skips the additions of the scalar's zero bits together instead
// of executing both sides of the branch.  In the last six stages the lanes take consecutive k (coalesced, divergent).  The
// factor 1 / N is appended: one more multiplication per point, (N / 2)(m - 1) + N in all.  Several transforms of one size
// (L1, LA, LB and H's) run as one launch per stage.  The conversion to affine is the shared-inversion kernel of setup.hip,
// once, at the end of the call (the column sums read XYZZ).
//
// H needs only the odd outputs of the 2n-point transform M of T1.  With g = w_2n:
//   M_{2j+1} = (1 / 2n) sum_{i<n} w_n^(-j i) D_i,   D_i = g^(-i) (T1_i - T1_{i+n}),
// so one pass forms D (n multiplications) and the n-point transform follows, with 1 / 2n as its appended factor.
//
// Column sums.  As in setup.hip, with points for values: one thread per segment of at most 64 terms forms sum coef P, one
// thread per wire adds its segments.  A term with coefficient +1 or -1 (most terms of a real circuit) is one addition; a
// general coefficient c above r / 2 is applied as -((r - c) P).  Three segment passes: L1 for all three matrices (A, B1, and
// C's part of K), LB for A's and LA for B's segments (the rest of K), L2 for B's segments (B2).
//
// delta.  C and H lie next to each other in the G1 list and are multiplied by 1 / delta in one launch, which delta = 1
// skips; delta1 and delta2 are the generators times delta.  delta and 1 / delta reach the kernels through a device buffer
// that is zeroed before it is released.
//
// Prepare (gwb_ptau_prepare_phase2: sections 12 to 15 from 2 to 5).  A Lagrange section holds every level m = 0 .. top, level m
// being Lag_m of the monomial section's first 2^m points.  The workspace of a section is the section's own layout in XYZZ:
// level m in the slots [2^m - 1, 2^(m+1) - 1).  The monomial prefix is uploaded once and load_kernel reads it once per level,
// bit-reversed for that level (the top level's launch reads every point and checks it).  idft_levels_stage_kernel then runs
// stage s of every level m > s in one launch, top launches for a section where level by level they would be top (top + 1) / 2.
// The twiddle of a butterfly, w_(2^(s+1))^(-k), depends on (s, k) and not on the level, so one table of 2^power values
// (w_(2^(power+1))^(-j), indexed k << (power - s)) serves every level of every section, and butterflies of different levels
// with one k can share a wave: with v = k 2^(top-s) + w they do while top - s >= 6, that is in every stage but the last five
// of the launch.  Level by level (idft_stage_kernel) only the levels m >= s + 7 have 64 groups to give a wave, so at stage s the
// levels s + 1 .. s + 6 run divergent there; here they fill the wave together (ptau_internal.hpp's level_butterfly has the
// decode, a count of leading zeros).  In the last five stages fewer than 63 butterflies have one k, and the lanes take
// consecutive k as before.  k = 0 has no multiplication.  scale_levels_kernel applies 1 / 2^m to the whole array in one
// launch, the level from the slot index and the power + 2 scalars from a small device table; a wave is inside one level from
// level 6 on, so its scalar is uniform.  The four sections run as four passes through one workspace, section 12 with its extra
// level (the missing last input is O) and no batching of the three G1 sections: the passes differ in length by one level, and
// one pass already fills the device from power 10 on.  Results leave through the shared-inversion kernel and come back in
// pieces of CWC_CONTRIBUTE_CHUNK points.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage for gfx950; every kernel: 0 bytes of scratch; VGPRs + AGPRs, waves / SIMD):
//   load_kernel<G1> 53, 8           load_kernel<G2> 110, 4            twiddle_kernel 36, 8        put_fr_kernel 10, 8
//   idft_stage_kernel<G1> 188, 2    idft_stage_kernel<G2> 256 + 170, 1     odd_half_kernel<G1> 152, 3
//   idft_levels_stage_kernel<G1> 188, 2    idft_levels_stage_kernel<G2> 256 + 170, 1
//   scale_levels_kernel<G1> 124, 4         scale_levels_kernel<G2> 256 + 14, 1
//   scale_kernel<G1> 114, 4         scale_kernel<G2> 256 + 1, 1
//   segments_kernel<G1> 186, 2      segments_kernel<G2> 256 + 151, 1
//   wires_g1_kernel 232, 2          wires_one_kernel<G2> 246, 2
// Launch bounds of 256 threads are one wave per SIMD, which leaves the allocator all 512 registers; the G2 butterfly holds the
// multiplicand, the accumulator and the other operand (64 registers each) across an inlined double-and-add.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/graph_witness_groth16_ptau.h"
#include "bn254_points_gfx950.hpp"
#include "groth16_internal.hpp"
#include "ptau_internal.hpp"
#include "setup_internal.hpp"

using namespace cwc_r1cs;
using namespace cwc_g16;
using namespace cwc_setup;
using cwc::Fr;

namespace {

constexpr uint32_t THREADS = 256;
constexpr uint32_t MAX_LOG_N = MAX_DOMAIN_POWER;
constexpr unsigned long long NO_FAULT = ~0ull;

// out[slot(i)] = the affine point in[first + i stride] in XYZZ form, slot(i) = i or, for rev_bits != 0, i's rev_bits bits
// reversed.  flag != nullptr: the point is checked, and the smallest 2 i + fault of the array is left in *flag.
template <class T>
__global__ __launch_bounds__(THREADS) void load_kernel(const uint8_t* __restrict__ in, uint32_t n, uint32_t first, uint32_t stride, uint32_t canonical,
                                                       uint32_t rev_bits, Xyzz<T>* __restrict__ out, unsigned long long* __restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<T> a;
    const bool in_range = get_coords<T>(in + ((size_t)first + (size_t)i * stride) * sizeof a, canonical != 0, a.x, a.y);
    Xyzz<T> p = from_affine(a);
    if (flag) {
        if (!in_range) {
            atomicMin(flag, 2ull * i + (uint32_t)PointFault::COORDINATE);
            p = xyzz_inf<T>();
        } else if (!xyzz_is_inf(p) && !on_curve(a, curve_b<T>())) {
            atomicMin(flag, 2ull * i + (uint32_t)PointFault::CURVE);
            p = xyzz_inf<T>();
        }
    }
    out[rev_bits ? __brev(i) >> (32 - rev_bits) : i] = p;
}

// out[k] = base^k, canonical, for k < count (bp.v[b] = base^(2^b))
__global__ __launch_bounds__(THREADS) void twiddle_kernel(Fr* __restrict__ out, uint32_t count, Pows bp) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    Fr x = cwc::fr_one();
    for (uint32_t b = 0; b <= MAX_LOG_N; ++b)
        if ((k >> b) & 1u) x = cwc::fr_mul(x, bp.v[b]);
    out[k] = cwc::fr_from_mont(x);
}

// stage s of `batch` transforms of 2^log_n points each, transform t in x[t 2^log_n ..); tw[k] = w_N^(-k) for k < N / 2
template <class T>
__global__ __launch_bounds__(THREADS) void idft_stage_kernel(Xyzz<T>* __restrict__ x, uint32_t log_n, uint32_t s, uint32_t batch,
                                                             const Fr* __restrict__ tw) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t per = 1u << (log_n - 1);  // butterflies per transform
    if (t >= (uint64_t)batch * per) return;
    const uint32_t u = (uint32_t)t & (per - 1), half = 1u << s, groups = per >> s;
    uint32_t k, grp;
    if (groups >= 64) {  // a wave: one k, 64 groups
        grp = u & (groups - 1);
        k = u >> (log_n - 1 - s);
    } else {
        k = u & (half - 1);
        grp = u >> s;
    }
    Xyzz<T>* lo = x + ((t >> (log_n - 1)) << log_n) + ((size_t)grp << (s + 1)) + k;
    const Xyzz<T> a = lo[0];
    Xyzz<T> c = lo[half];
    if (k) c = xyzz_mul_short(c, tw[(size_t)k * groups]);
    lo[0] = xyzz_add(a, c);
    lo[half] = xyzz_add(a, xyzz_neg(c));
}

// d[bitrev(i)] = g^(-i) (t[i] - t[i + n]) for i < n = 2^log_n; twg[i] = g^(-i)
template <class T>
__global__ __launch_bounds__(THREADS) void odd_half_kernel(const Xyzz<T>* __restrict__ t, uint32_t log_n, const Fr* __restrict__ twg,
                                                           Xyzz<T>* __restrict__ d) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, n = 1u << log_n;
    if (i >= n) return;
    Xyzz<T> c = xyzz_add(t[i], xyzz_neg(t[(size_t)i + n]));
    if (i) c = xyzz_mul_short(c, twg[i]);
    d[__brev(i) >> (32 - log_n)] = c;
}

// *out = v: a scalar for scale_kernel, without a copy from host memory that the stream would have to wait for
__global__ __launch_bounds__(64) void put_fr_kernel(Fr* __restrict__ out, Fr v) {
    if (threadIdx.x == 0) *out = v;
}

// x[i] = k x[i] for i < count
template <class T>
__global__ __launch_bounds__(THREADS) void scale_kernel(Xyzz<T>* __restrict__ x, uint32_t count, const Fr* __restrict__ k) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    x[i] = xyzz_mul_short(x[i], *k);
}

// Stage s of the transforms of every level m in (s, top] of one section (the header's "Prepare"; ptau_internal.hpp's
// level_butterfly has the thread layout): x holds level m in the slots [2^m - 1, 2^(m+1) - 1), inputs bit-reversed per level;
// tw[j] = w_N^(-j) for one N >= 2^top, and tw_shift = log2(N) - 1 - s, so that tw[k << tw_shift] = w_(2 half)^(-k) whatever
// the level.  2^top threads.
template <class T>
__global__ __launch_bounds__(THREADS) void idft_levels_stage_kernel(Xyzz<T>* __restrict__ x, uint32_t top, uint32_t s, uint32_t tw_shift,
                                                                    const Fr* __restrict__ tw) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    cwc_ptau::LevelButterfly b;
    if ((v >> top) != 0 || !cwc_ptau::level_butterfly(v, top, s, b)) return;
    const uint32_t half = 1u << s;
    Xyzz<T>* lo = x + (((size_t)1 << b.m) - 1) + ((size_t)b.grp << (s + 1)) + b.k;
    const Xyzz<T> a = lo[0];
    Xyzz<T> c = lo[half];
    if (b.k) c = xyzz_mul_short(c, tw[(size_t)b.k << tw_shift]);
    lo[0] = xyzz_add(a, c);
    lo[half] = xyzz_add(a, xyzz_neg(c));
}

// x[i] = inv[m] x[i] for the slots i < count of the levels m = floor(log2(i + 1)) >= 1: the factor 1 / 2^m of every level, canonical
template <class T>
__global__ __launch_bounds__(THREADS) void scale_levels_kernel(Xyzz<T>* __restrict__ x, uint32_t count, const Fr* __restrict__ inv) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t m = 31u - (uint32_t)__builtin_clz(i + 1u);
    if (m) x[i] = xyzz_mul_short(x[i], inv[m]);
}

// part[s] = sum of coefficient x pts[constraint] over the terms ent[seg_off[s] .. seg_off[s + 1]) of one (wire, matrix)
// column; the points of matrix m are pm (nullptr: the pass leaves this matrix out, part[s] = O)
template <class T>
__global__ __launch_bounds__(THREADS) void segments_kernel(const uint32_t* __restrict__ ent, const uint32_t* __restrict__ cidx,
                                                           const Fr* __restrict__ coef, const uint32_t* __restrict__ seg_off,
                                                           const uint32_t* __restrict__ seg_key, uint32_t n_seg, const Xyzz<T>* __restrict__ p0,
                                                           const Xyzz<T>* __restrict__ p1, const Xyzz<T>* __restrict__ p2,
                                                           Xyzz<T>* __restrict__ part) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    const uint32_t m = seg_key[s] % 3u;
    const Xyzz<T>* pts = m == 0 ? p0 : m == 1 ? p1 : p2;
    Xyzz<T> acc = xyzz_inf<T>();
    if (pts) {
        Fr half_r = cwc::fr_p();  // (r - 1) / 2
        half_r = cwc::u256_shr(half_r, 1);
        for (uint32_t j = seg_off[s], end = seg_off[s + 1]; j < end; ++j) {
            const uint32_t e = ent[j], kind = e >> 30;
            Xyzz<T> q = pts[e & WIRE_MASK];
            bool minus = kind == KIND_MINUS;
            if (kind == KIND_GENERAL) {
                Fr c = cwc::fr_from_mont(coef[cidx[j]]);
                minus = cwc::u256_lt(half_r, c);
                Fr nc;
                cwc::u256_sub(nc, cwc::fr_p(), c);
                c = cwc::u256_select(minus, nc, c);
                q = xyzz_mul_short(q, c);
            }
            acc = xyzz_add(acc, minus ? xyzz_neg(q) : q);
        }
    }
    part[s] = acc;
}

// The G1 points of wire i from its segments (seg_key = 3 wire + matrix): pa holds the L1 pass (A, B1 and C's part of K), pk
// the LB / LA pass (the rest of K).  list = [A: nW][B1: nW][C: nW - nPub - 1][H: n][IC: nPub + 1][delta1]; K goes to IC or C.
__global__ __launch_bounds__(THREADS) void wires_g1_kernel(const Xyzz<G1>* __restrict__ pa, const Xyzz<G1>* __restrict__ pk,
                                                           const uint32_t* __restrict__ seg_key, const uint32_t* __restrict__ wire_seg,
                                                           const Xyzz<G1>* __restrict__ l1, const Xyzz<G1>* __restrict__ lb, uint32_t n_wires,
                                                           uint32_t n_constraints, uint32_t n_pub, uint32_t n, Xyzz<G1>* __restrict__ list) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_wires) return;
    Xyzz<G1> a = xyzz_inf<G1>(), b = a, k = a;
    for (uint32_t s = wire_seg[i], end = wire_seg[i + 1]; s < end; ++s) {
        const uint32_t m = seg_key[s] - 3u * i;
        const Xyzz<G1> p = pa[s];
        if (m == 2) {
            k = xyzz_add(k, p);
        } else {
            k = xyzz_add(k, pk[s]);
            if (m == 0)
                a = xyzz_add(a, p);
            else
                b = xyzz_add(b, p);
        }
    }
    if (i <= n_pub) {
        a = xyzz_add(a, l1[n_constraints + i]);
        k = xyzz_add(k, lb[n_constraints + i]);
    }
    const KeyLayout at{n_wires, n_pub, n};
    list[i] = a;
    list[at.b1() + i] = b;
    list[i <= n_pub ? at.ic() + i : at.c() + (i - n_pub - 1)] = k;
}

// out[i] = the sum of wire i's segments of matrix m
template <class T>
__global__ __launch_bounds__(THREADS) void wires_one_kernel(const Xyzz<T>* __restrict__ part, const uint32_t* __restrict__ seg_key,
                                                            const uint32_t* __restrict__ wire_seg, uint32_t n_wires, uint32_t m,
                                                            Xyzz<T>* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_wires) return;
    Xyzz<T> acc = xyzz_inf<T>();
    for (uint32_t s = wire_seg[i], end = wire_seg[i + 1]; s < end; ++s)
        if (seg_key[s] - 3u * i == m) acc = xyzz_add(acc, part[s]);
    out[i] = acc;
}

// ---- host -----------------------------------------------------------------------------------------------------------------

Fr inverse_of_u32(uint32_t x) {  // canonical 1 / x mod r
    return cwc::fr_from_mont(cwc::fr_inv_fermat(cwc::fr_to_mont(Fr{{x, 0, 0, 0, 0, 0, 0, 0}})));
}

// tw[k] = w_N^(-k) for k < N / 2, N = 2^log_n
void enqueue_twiddles(Fr* tw, uint32_t log_n, hipStream_t s) {
    Fr wn, g;
    qap_roots(log_n, wn, g);
    const uint32_t count = 1u << (log_n - 1);
    hipLaunchKernelGGL(twiddle_kernel, dim3(blocks_for(count, THREADS)), dim3(THREADS), 0, s, tw, count, powers_of(cwc::fr_inv_fermat(wn)));
}

template <class T>
void enqueue_load(const uint8_t* d_in, uint32_t n, uint32_t first, uint32_t stride, bool canonical, uint32_t rev_bits, Xyzz<T>* out,
                  unsigned long long* flag, hipStream_t s) {
    hipLaunchKernelGGL(load_kernel<T>, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, s, d_in, n, first, stride, canonical ? 1u : 0u, rev_bits, out, flag);
}

// the stages of `batch` transforms in x (inputs in bit-reversed slots), without the factor 1 / N
template <class T>
void enqueue_stages(Xyzz<T>* x, uint32_t log_n, uint32_t batch, const Fr* tw, hipStream_t s) {
    const uint64_t threads = (uint64_t)batch << (log_n - 1);
    for (uint32_t st = 0; st < log_n; ++st)
        hipLaunchKernelGGL(idft_stage_kernel<T>, dim3(blocks_for(threads, THREADS)), dim3(THREADS), 0, s, x, log_n, st, batch, tw);
}

template <class T>
void enqueue_scale(Xyzz<T>* x, uint32_t count, const Fr* d_k, hipStream_t s) {
    if (count) hipLaunchKernelGGL(scale_kernel<T>, dim3(blocks_for(count, THREADS)), dim3(THREADS), 0, s, x, count, d_k);
}

struct Delta {
    Fr delta, delta_inv;  // canonical
    ~Delta() { explicit_bzero(this, sizeof *this); }
};

bool take_delta(const uint8_t* given, Delta& d, std::string& err) {
    if (given) {
        memcpy(d.delta.v, given, 32);
        if (cwc::u256_is_zero(d.delta) || !cwc::u256_lt(d.delta, cwc::fr_p())) {
            err = "groth16 setup: delta is not in [1, r)";
            return false;
        }
    } else {
        do {
            if (!draw_fr(d.delta, err)) return false;
        } while (cwc::u256_is_zero(d.delta));
    }
    d.delta_inv = cwc::fr_from_mont(cwc::fr_inv_fermat(cwc::fr_to_mont(d.delta)));
    return true;
}

PhaseTimes<7> g_phases;

// an array of points that the device loads and checks: where its indices lie in the file, for the message
struct Checked {
    uint32_t section;
    uint64_t base;
    uint32_t first, stride;
    bool g2;
};

int setup(gwb_r1cs* r, const uint8_t* ptau, size_t ptau_len, const uint8_t* delta, uint32_t mode, void** zkey, size_t* zkey_len, gw_status_t* status) {
    gwb_r1cs_qap_info_t qi;
    if (gwb_r1cs_qap_info(r, &qi, status) != 0) return 1;
    const uint32_t p = qi.domain_power, n = (uint32_t)qi.domain_size;
    const uint32_t nw = r->info.n_wires, nc = r->info.n_constraints, n_pub = r->info.n_pub_out + r->info.n_pub_in;
    std::string err;
    cwc_ptau::View view;
    cwc_ptau::Plan pl;
    if (!cwc_ptau::parse(ptau, ptau_len, view, err) || !cwc_ptau::plan(view, p, mode, pl, err) || !cwc_ptau::check_header_points(pl, err))
        return fail(status, err);
    Delta dl;
    if (!take_delta(delta, dl, err)) return fail(status, err);
    const bool delta_is_one = cwc::u256_eq(dl.delta, Fr{{1, 0, 0, 0, 0, 0, 0, 0}});
    const KeyLayout at{nw, n_pub, n};
    const uint64_t n1 = at.n1() + 1, n2 = (uint64_t)nw + 1;  // [A][B1][C][H][IC][delta1], [B2][delta2]
    if (n1 > 0x7fffffffull) return fail(status, "groth16 setup: more than 2^31 - 1 points");
    std::vector<uint8_t> sec4;
    if (!coefficients_section(r, sec4, err)) return fail(status, err);
    Columns col;
    transpose(r, segment_terms(), col);
    const uint32_t n_seg = (uint32_t)col.seg_key.size();
    const size_t X1 = sizeof(Xyzz<G1>), X2 = sizeof(Xyzz<G2>);
    const size_t off_c = at.c(), off_h = at.h();

    SetupDevice<8> D;
    Carve cw;
    const size_t o_col = cw.take(columns_bytes(col, r->sys.coef.size())),
                 o_raw1 = cw.take(5ull * n * G1_BYTES),  // compute: T1 (2n), AT, BT; file: L1, LA, LB, M (2n)
                 o_raw2 = cw.take((size_t)n * G2_BYTES), o_lag1 = cw.take(4ull * n * X1),  // L1, LA, LB and (compute) D
                 o_t1 = cw.take(pl.from_file ? 0 : 2ull * n * X1), o_lag2 = cw.take((size_t)n * X2), o_tw = cw.take((size_t)n / 2 * 32),
                 o_twg = cw.take((size_t)n * 32), o_pa = cw.take((size_t)n_seg * X1), o_pk = cw.take((size_t)n_seg * X1),
                 o_pq = cw.take((size_t)n_seg * X2), o_x1 = cw.take(n1 * X1), o_x2 = cw.take(n2 * X2), o_p1 = cw.take(n1 * G1_BYTES),
                 o_p2 = cw.take(n2 * G2_BYTES), o_flag = cw.take(8 * sizeof(unsigned long long)), o_pub = cw.take(2 * 32);
    hipError_t e = D.open(256, cw.o);
    if (e != hipSuccess) return fail(status, hip_err("allocating the setup workspace", e));
    uint8_t* W = D.work.as<uint8_t>();
    auto up = [&](size_t off, const void* src, size_t bytes) {
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(W + off, src, bytes, hipMemcpyHostToDevice, D.s);
    };
    const DeviceColumns dc = upload_columns(col, r->sys.coef, W + o_col, D.s, e);
    const size_t nb1 = (size_t)n * G1_BYTES;
    if (pl.from_file) {
        up(o_raw1, pl.l1, nb1);
        up(o_raw1 + nb1, pl.la, nb1);
        up(o_raw1 + 2 * nb1, pl.lb, nb1);
        up(o_raw1 + 3 * nb1, pl.m, 2 * nb1);
        up(o_raw2, pl.l2, (size_t)n * G2_BYTES);
    } else {
        up(o_raw1, pl.t1, 2 * nb1);
        up(o_raw1 + 2 * nb1, pl.at, nb1);
        up(o_raw1 + 3 * nb1, pl.bt, nb1);
        up(o_raw2, pl.t2, (size_t)n * G2_BYTES);
    }
    // the generators, which delta1 and delta2 are multiples of, at the end of the two lists
    const Xyzz<G1> gen1 = from_affine(g1_generator());
    const Xyzz<G2> gen2 = from_affine(g2_generator());
    uint8_t gb2[G2_BYTES];  // gamma2 of a key without a trapdoor
    put_coords<G2>(gb2, gen2.X, gen2.Y, false);
    up(o_x1 + (n1 - 1) * X1, &gen1, X1);
    up(o_x2 + (n2 - 1) * X2, &gen2, X2);
    const Fr pub[2] = {inverse_of_u32(n), inverse_of_u32(2 * n)};
    up(o_pub, pub, sizeof pub);
    if (e == hipSuccess) e = hipMemsetAsync(W + o_flag, 0xff, 8 * sizeof(unsigned long long), D.s);
    if (e == hipSuccess) e = hipMemcpyAsync(D.secret.as(), &dl, sizeof dl, hipMemcpyHostToDevice, D.s);
    if (e == hipSuccess) e = hipStreamSynchronize(D.s);  // the copies have left the host arrays
    if (e != hipSuccess) return fail(status, hip_err("uploading the ceremony points and the transposed constraint matrices", e));
    const Fr *d_delta = D.secret.as<const Fr>(), *d_delta_inv = d_delta + 1, *d_inv_n = (const Fr*)(W + o_pub), *d_inv_2n = d_inv_n + 1;

    Xyzz<G1>*lag1 = (Xyzz<G1>*)(W + o_lag1), *l1 = lag1, *la = lag1 + n, *lb = lag1 + 2 * (size_t)n, *dd = lag1 + 3 * (size_t)n;
    Xyzz<G1>*t1 = (Xyzz<G1>*)(W + o_t1), *x1 = (Xyzz<G1>*)(W + o_x1);
    Xyzz<G2>*l2 = (Xyzz<G2>*)(W + o_lag2), *x2 = (Xyzz<G2>*)(W + o_x2);
    unsigned long long* flag = (unsigned long long*)(W + o_flag);
    Fr *tw = (Fr*)(W + o_tw), *twg = (Fr*)(W + o_twg);
    std::vector<Checked> checked;
    D.ev.record(0, D.s);
    if (pl.from_file) {
        const uint64_t lvl = (uint64_t)n - 1;
        checked = {{12, lvl, 0, 1, false}, {14, lvl, 0, 1, false}, {15, lvl, 0, 1, false}, {12, 2 * (uint64_t)n - 1, 1, 2, false}, {13, lvl, 0, 1, true}};
        enqueue_load<G1>(W + o_raw1, n, 0, 1, false, 0, l1, flag + 0, D.s);
        enqueue_load<G1>(W + o_raw1 + nb1, n, 0, 1, false, 0, la, flag + 1, D.s);
        enqueue_load<G1>(W + o_raw1 + 2 * nb1, n, 0, 1, false, 0, lb, flag + 2, D.s);
        enqueue_load<G1>(W + o_raw1 + 3 * nb1, n, 1, 2, false, 0, x1 + off_h, flag + 3, D.s);  // M's odd points: H before delta
        enqueue_load<G2>(W + o_raw2, n, 0, 1, false, 0, l2, flag + 4, D.s);
    } else {
        checked = {{2, 0, 0, 1, false}, {4, 0, 0, 1, false}, {5, 0, 0, 1, false}, {3, 0, 0, 1, true}};
        enqueue_load<G1>(W + o_raw1, 2 * n, 0, 1, false, 0, t1, flag + 0, D.s);
        enqueue_load<G1>(W + o_raw1, n, 0, 1, false, p, l1, nullptr, D.s);  // T1's first half again, to the transform's slots
        enqueue_load<G1>(W + o_raw1 + 2 * nb1, n, 0, 1, false, p, la, flag + 1, D.s);
        enqueue_load<G1>(W + o_raw1 + 3 * nb1, n, 0, 1, false, p, lb, flag + 2, D.s);
        enqueue_load<G2>(W + o_raw2, n, 0, 1, false, p, l2, flag + 3, D.s);
    }
    D.ev.record(1, D.s);
    if (!pl.from_file) {
        Fr wn, g;
        qap_roots(p, wn, g);
        enqueue_twiddles(tw, p, D.s);
        hipLaunchKernelGGL(twiddle_kernel, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, D.s, twg, n, powers_of(cwc::fr_inv_fermat(g)));
        hipLaunchKernelGGL(odd_half_kernel<G1>, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, D.s, (const Xyzz<G1>*)t1, p, (const Fr*)twg, dd);
        enqueue_stages<G1>(lag1, p, 4, tw, D.s);
        enqueue_scale<G1>(lag1, 3 * n, d_inv_n, D.s);
        enqueue_scale<G1>(dd, n, d_inv_2n, D.s);
        e = hipMemcpyAsync(x1 + off_h, dd, (size_t)n * X1, hipMemcpyDeviceToDevice, D.s);
        if (e != hipSuccess) return fail(status, hip_err("placing H", e));
    }
    D.ev.record(2, D.s);
    if (!pl.from_file) {
        enqueue_stages<G2>(l2, p, 1, tw, D.s);
        enqueue_scale<G2>(l2, n, d_inv_n, D.s);
    }
    D.ev.record(3, D.s);
    Xyzz<G1>*pa = (Xyzz<G1>*)(W + o_pa), *pk = (Xyzz<G1>*)(W + o_pk);
    Xyzz<G2>* pq = (Xyzz<G2>*)(W + o_pq);
    const Xyzz<G1>* none1 = nullptr;
    const Xyzz<G2>* none2 = nullptr;
    if (n_seg) {
        hipLaunchKernelGGL(segments_kernel<G1>, dim3(blocks_for(n_seg, THREADS)), dim3(THREADS), 0, D.s, dc.ent, dc.cidx, dc.coef, dc.seg_off, dc.seg_key, n_seg,
                           (const Xyzz<G1>*)l1, (const Xyzz<G1>*)l1, (const Xyzz<G1>*)l1, pa);
        hipLaunchKernelGGL(segments_kernel<G1>, dim3(blocks_for(n_seg, THREADS)), dim3(THREADS), 0, D.s, dc.ent, dc.cidx, dc.coef, dc.seg_off, dc.seg_key, n_seg,
                           (const Xyzz<G1>*)lb, (const Xyzz<G1>*)la, none1, pk);
    }
    hipLaunchKernelGGL(wires_g1_kernel, dim3(blocks_for(nw, THREADS)), dim3(THREADS), 0, D.s, (const Xyzz<G1>*)pa, (const Xyzz<G1>*)pk, dc.seg_key, dc.wire_seg,
                       (const Xyzz<G1>*)l1, (const Xyzz<G1>*)lb, nw, nc, n_pub, n, x1);
    D.ev.record(4, D.s);
    if (n_seg)
        hipLaunchKernelGGL(segments_kernel<G2>, dim3(blocks_for(n_seg, THREADS)), dim3(THREADS), 0, D.s, dc.ent, dc.cidx, dc.coef, dc.seg_off, dc.seg_key, n_seg, none2,
                           (const Xyzz<G2>*)l2, none2, pq);
    hipLaunchKernelGGL(wires_one_kernel<G2>, dim3(blocks_for(nw, THREADS)), dim3(THREADS), 0, D.s, (const Xyzz<G2>*)pq, dc.seg_key, dc.wire_seg, nw, 1u, x2);
    D.ev.record(5, D.s);
    if (!delta_is_one) enqueue_scale<G1>(x1 + off_c, (nw - n_pub - 1) + n, d_delta_inv, D.s);  // C and H
    enqueue_scale<G1>(x1 + (n1 - 1), 1, d_delta, D.s);
    enqueue_scale<G2>(x2 + (n2 - 1), 1, d_delta, D.s);
    D.ev.record(6, D.s);
    enqueue_affine_g1(x1, (uint32_t)n1, W + o_p1, false, D.s);
    enqueue_affine_g2(x2, (uint32_t)n2, W + o_p2, false, D.s);
    D.ev.record(7, D.s);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(status, hip_err("launching the setup kernels", e));
    std::vector<uint8_t> p1(n1 * G1_BYTES), p2(n2 * G2_BYTES);
    unsigned long long faults[8];
    e = hipMemcpyAsync(p1.data(), W + o_p1, p1.size(), hipMemcpyDeviceToHost, D.s);
    if (e == hipSuccess) e = hipMemcpyAsync(p2.data(), W + o_p2, p2.size(), hipMemcpyDeviceToHost, D.s);
    if (e == hipSuccess) e = hipMemcpyAsync(faults, flag, sizeof faults, hipMemcpyDeviceToHost, D.s);
    if (e == hipSuccess) e = hipMemsetAsync(D.secret.as(), 0, D.secret_bytes, D.s);
    if (e == hipSuccess) e = hipStreamSynchronize(D.s);
    if (e != hipSuccess) return fail(status, hip_err("running the setup", e));
    for (size_t a = 0; a < checked.size(); ++a)
        if (faults[a] != NO_FAULT) {
            const Checked& c = checked[a];
            return fail(status, cwc_ptau::point_message(c.section, c.base + c.first + (faults[a] >> 1) * c.stride, (PointFault)(faults[a] & 1), c.g2));
        }
    g_phases.record(D.ev, pl.from_file ? 6u : 0u);  // from a file, nothing lies between the events of the two transforms
    const uint8_t *a = p1.data(), *b1 = a + at.b1() * G1_BYTES, *c = a + off_c * G1_BYTES, *h = a + off_h * G1_BYTES,
                  *ic = a + at.ic() * G1_BYTES, *delta1 = a + at.n1() * G1_BYTES;
    const uint8_t *b2 = p2.data(), *delta2 = b2 + (size_t)nw * G2_BYTES;
    const KeyPoints kp{nw, n_pub, n, pl.at, pl.bt, pl.beta2, gb2, delta1, delta2, ic, a, b1, b2, c, h};
    return write_zkey(kp, sec4, zkey, zkey_len, status);
}

template <class T>
int idft_aid(const void* d_points, uint32_t log_n, void* d_out, hipStream_t s, gw_status_t* status) {
    const uint32_t n = 1u << log_n;
    Carve cw;
    const size_t o_x = cw.take((size_t)n * sizeof(Xyzz<T>)), o_tw = cw.take((size_t)n / 2 * 32), o_k = cw.take(32);
    void* ws = nullptr;
    hipError_t e = hipMallocAsync(&ws, cw.o, s);
    if (e != hipSuccess) return fail(status, hip_err("allocating the transform's workspace", e));
    uint8_t* W = (uint8_t*)ws;
    Xyzz<T>* x = (Xyzz<T>*)(W + o_x);
    Fr *tw = (Fr*)(W + o_tw), *k = (Fr*)(W + o_k);
    enqueue_load<T>((const uint8_t*)d_points, n, 0, 1, true, log_n, x, nullptr, s);
    enqueue_twiddles(tw, log_n, s);
    hipLaunchKernelGGL(put_fr_kernel, dim3(1), dim3(64), 0, s, k, inverse_of_u32(n));
    enqueue_stages<T>(x, log_n, 1, tw, s);
    enqueue_scale<T>(x, n, k, s);
    if (sizeof(typename T::E) == 32)
        enqueue_affine_g1(x, n, (uint8_t*)d_out, true, s);
    else
        enqueue_affine_g2(x, n, (uint8_t*)d_out, true, s);
    e = hipGetLastError();
    const hipError_t ef = hipFreeAsync(ws, s);
    if (e != hipSuccess) return fail(status, hip_err("launching the transform", e));
    if (ef != hipSuccess) return fail(status, hip_err("releasing the transform's workspace", ef));
    set_ok(status);
    return 0;
}

// ---- prepare phase 2: sections 12 to 15 from sections 2 to 5 -------------------------------------------------------------------

PhaseTimes<4> g_prepare_phases;  // load, idft_g1, idft_g2, affine: summed over the four section passes

struct PrepareDevice {
    Stream s;
    PhaseEvents<4> ev;
    DeviceBuf work;
    size_t raw = 0, x = 0, tw = 0, inv = 0, out = 0, flag = 0;  // offsets into work
};

// One section pass: the first 2^top points of section id - 10 -> the 2^(top+1) - 1 points of section id at `body`, through the
// device in pieces of `chunk` points; ms gets the pass's times.  err: a point fault in point_message's words, or the runtime's.
template <class T>
bool lagrange_section(const cwc_ptau::View& view, uint32_t id, PrepareDevice& D, uint64_t chunk, uint8_t* body, float (&ms)[4], bool& timed,
                      std::string& err) {
    constexpr bool g2 = sizeof(typename T::E) != 32;
    constexpr size_t PB = g2 ? G2_BYTES : G1_BYTES;
    const uint32_t src = id - 10, top = cwc_ptau::top_level(view, id);
    const uint64_t n_in = view.sec[src].size / PB, slots = (2ull << top) - 1;  // n_in = 2^top, or one fewer in section 2
    uint8_t* W = D.work.as<uint8_t>();
    Xyzz<T>* x = (Xyzz<T>*)(W + D.x);
    unsigned long long* flag = (unsigned long long*)(W + D.flag);
    D.ev.record(0, D.s);
    hipError_t e = hipMemcpyAsync(W + D.raw, view.sec[src].p, n_in * PB, hipMemcpyHostToDevice, D.s);
    if (e == hipSuccess && n_in < (1ull << top)) e = hipMemsetAsync(W + D.raw + n_in * PB, 0, PB, D.s);  // the missing last input: O
    if (e == hipSuccess) e = hipMemsetAsync(flag, 0xff, sizeof *flag, D.s);
    if (e != hipSuccess) {
        err = hip_err("uploading a section of ceremony points", e);
        return false;
    }
    for (uint32_t m = 0; m <= top; ++m)  // the top level reads every point: it checks them
        enqueue_load<T>(W + D.raw, 1u << m, 0, 1, false, m, x + (((size_t)1 << m) - 1), m == top ? flag : nullptr, D.s);
    D.ev.record(1, D.s);
    for (uint32_t st = 0; st < top; ++st)
        hipLaunchKernelGGL(idft_levels_stage_kernel<T>, dim3(blocks_for(1ull << top, THREADS)), dim3(THREADS), 0, D.s, x, top, st, view.power - st,
                           (const Fr*)(W + D.tw));
    hipLaunchKernelGGL(scale_levels_kernel<T>, dim3(blocks_for(slots, THREADS)), dim3(THREADS), 0, D.s, x, (uint32_t)slots, (const Fr*)(W + D.inv));
    D.ev.record(2, D.s);
    unsigned long long fault = NO_FAULT;
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&fault, flag, sizeof fault, hipMemcpyDeviceToHost, D.s);
    for (uint64_t at = 0; at < slots && e == hipSuccess; at += chunk) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, slots - at);
        if (g2)
            enqueue_affine_g2(x + at, m, W + D.out, false, D.s);
        else
            enqueue_affine_g1(x + at, m, W + D.out, false, D.s);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(body + at * PB, W + D.out, (size_t)m * PB, hipMemcpyDeviceToHost, D.s);
        if (e == hipSuccess) e = hipStreamSynchronize(D.s);  // the piece's buffer is written again by the next piece
        if (e == hipSuccess && fault != NO_FAULT) {
            err = cwc_ptau::point_message(src, fault >> 1, (PointFault)(fault & 1), g2);
            return false;
        }
    }
    D.ev.record(3, D.s);
    if (e != hipSuccess) {
        err = hip_err("transforming a section of ceremony points", e);
        return false;
    }
    float t[3];
    if (D.ev.elapsed(t) == hipSuccess) {
        ms[0] += t[0];
        ms[g2 ? 2 : 1] += t[1];
        ms[3] += t[2];
    } else {
        timed = false;
    }
    return true;
}

void put_u32(uint8_t* at, uint32_t v) { memcpy(at, &v, 4); }
void put_u64(uint8_t* at, uint64_t v) { memcpy(at, &v, 8); }

int prepare(const uint8_t* ptau, size_t len, void** out, size_t* out_len, gw_status_t* status) {
    std::string err;
    cwc_ptau::View view;
    if (!cwc_ptau::parse(ptau, len, view, err)) return fail(status, err);
    const uint32_t power = view.power;
    if (power > MAX_LOG_N)
        return fail(status, "ptau prepare: power " + std::to_string(power) + " is above " + std::to_string(MAX_LOG_N) + ", the largest whose top level has a root of unity here");
    const uint64_t np = 1ull << power;
    // the workspace: the largest all-level array (section 12's 4 np - 1 G1 points against section 13's 2 np - 1 G2 points), the
    // uploaded prefix, the twiddles and one piece of output
    const uint64_t x_bytes = std::max((4 * np - 1) * sizeof(Xyzz<G1>), (2 * np - 1) * sizeof(Xyzz<G2>)), cap = groth16_workspace_cap();
    const uint64_t chunk = std::min(piece_points("CWC_CONTRIBUTE_CHUNK"), 4 * np - 1);
    PrepareDevice D;
    Carve cw;
    D.raw = cw.take(2 * np * G1_BYTES);  // = np G2 points
    D.x = cw.take(x_bytes);
    D.tw = cw.take(np * 32);
    D.inv = cw.take((power + 2) * 32);
    D.out = cw.take(chunk * G2_BYTES);
    D.flag = cw.take(sizeof(unsigned long long));
    if (cw.o > cap)
        return fail(status, "ptau prepare: power " + std::to_string(power) + " needs " + std::to_string(cw.o) + " bytes of device workspace (" +
                                std::to_string(x_bytes) + " of them for all levels of one section), above the " + std::to_string(cap) +
                                " of CWC_GROTH16_WORKSPACE_MB (an out-of-core transform is not supported)");
    // the image: the input's sections other than 12 to 15 in its order, then 12 to 15
    const uint64_t lag_points[4] = {4 * np - 1, 2 * np - 1, 2 * np - 1, 2 * np - 1};
    uint64_t total = 12;
    uint32_t n_out = 4;
    for (const BinEntry& sct : view.order)
        if (sct.id < 12 || sct.id > 15) {
            total += 12 + sct.size;
            ++n_out;
        }
    uint64_t lag_off[4];
    for (int k = 0; k < 4; ++k) {
        lag_off[k] = total + 12;
        total += 12 + lag_points[k] * (k == 1 ? G2_BYTES : G1_BYTES);
    }
    struct Free {
        void operator()(void* p) const { free(p); }
    };
    std::unique_ptr<uint8_t, Free> img((uint8_t*)malloc(total));
    if (!img) return fail(status, "ptau prepare: out of host memory");
    uint8_t* o = img.get();
    memcpy(o, ptau, 8);
    put_u32(o + 8, n_out);
    uint64_t w = 12;
    for (const BinEntry& sct : view.order)
        if (sct.id < 12 || sct.id > 15) {
            put_u32(o + w, sct.id);
            put_u64(o + w + 4, sct.size);
            memcpy(o + w + 12, sct.p, sct.size);
            w += 12 + sct.size;
        }
    for (int k = 0; k < 4; ++k) {
        put_u32(o + lag_off[k] - 12, 12 + k);
        put_u64(o + lag_off[k] - 8, lag_points[k] * (k == 1 ? G2_BYTES : G1_BYTES));
    }

    hipError_t e = D.s.create();
    if (e == hipSuccess) e = D.ev.on();
    if (e == hipSuccess) e = D.work.alloc(cw.o);
    if (e != hipSuccess) return fail(status, hip_err("allocating the workspace of the Lagrange sections", e));
    uint8_t* W = D.work.as<uint8_t>();
    // tw[j] = w_(2 np)^(-j) for j < np: every level of every section takes its twiddles from it; inv[m] = 1 / 2^m = r - (r - 1) / 2^m
    Fr wn, g, rm1 = cwc::fr_p();
    qap_roots(power, wn, g);
    rm1.v[0] -= 1;
    std::vector<Fr> inv(power + 2, Fr{{1, 0, 0, 0, 0, 0, 0, 0}});
    for (uint32_t m = 1; m < power + 2; ++m) cwc::u256_sub(inv[m], cwc::fr_p(), cwc::u256_shr(rm1, m));
    hipLaunchKernelGGL(twiddle_kernel, dim3(blocks_for(np, THREADS)), dim3(THREADS), 0, D.s, (Fr*)(W + D.tw), (uint32_t)np, powers_of(cwc::fr_inv_fermat(g)));
    e = hipMemcpyAsync(W + D.inv, inv.data(), inv.size() * 32, hipMemcpyHostToDevice, D.s);
    if (e == hipSuccess) e = hipStreamSynchronize(D.s);  // the copy has left the host array
    if (e != hipSuccess) return fail(status, hip_err("making the twiddles of the Lagrange sections", e));
    float ms[4] = {0, 0, 0, 0};
    bool timed = true;
    for (int k = 0; k < 4; ++k) {
        const bool ok = k == 1 ? lagrange_section<G2>(view, 12 + k, D, chunk, o + lag_off[k], ms, timed, err)
                               : lagrange_section<G1>(view, 12 + k, D, chunk, o + lag_off[k], ms, timed, err);
        if (!ok) return fail(status, err);
    }
    g_prepare_phases.store(ms, timed);
    *out = img.release();
    *out_len = total;
    set_ok(status);
    return 0;
}

}  // namespace

extern "C" {

int gwb_ptau_prepare_phase2(const void* ptau, size_t ptau_len, void** out, size_t* out_len, gw_status_t* status) {
    if (!out || !out_len || (!ptau && ptau_len)) return fail(status, "gwb_ptau_prepare_phase2: NULL argument");
    *out = nullptr;
    *out_len = 0;
    try {
        return prepare((const uint8_t*)ptau, ptau_len, out, out_len, status);
    } catch (const std::bad_alloc&) {
        return fail(status, "ptau prepare: out of host memory");
    }
}

int gwb_ptau_prepare_phase_ms(float* ms) { return g_prepare_phases.read(ms); }

int gwb_groth16_setup_ptau(gwb_r1cs_t* r, const void* ptau, size_t ptau_len, const uint8_t* delta, uint32_t lagrange_mode, void** zkey,
                           size_t* zkey_len, gw_status_t* status) {
    if (!r || !zkey || !zkey_len || (!ptau && ptau_len)) return fail(status, "gwb_groth16_setup_ptau: NULL argument");
    *zkey = nullptr;
    *zkey_len = 0;
    try {
        return setup(r, (const uint8_t*)ptau, ptau_len, delta, lagrange_mode, zkey, zkey_len, status);
    } catch (const std::bad_alloc&) {
        return fail(status, "groth16 setup: out of host memory");
    }
}

int gwb_bn254_point_idft_batch_device(const void* d_points, uint32_t log_n, uint32_t group, void* d_out, void* hip_stream, gw_status_t* status) {
    if (!d_points || !d_out) return fail(status, "gwb_bn254_point_idft_batch_device: NULL argument");
    if (group != 1 && group != 2) return fail(status, "gwb_bn254_point_idft_batch_device: group " + std::to_string(group) + " (1 or 2 expected)");
    if (log_n < 1 || log_n > MAX_LOG_N)
        return fail(status, "gwb_bn254_point_idft_batch_device: log_n " + std::to_string(log_n) + " (1 to " + std::to_string(MAX_LOG_N) + " expected)");
    return group == 1 ? idft_aid<G1>(d_points, log_n, d_out, (hipStream_t)hip_stream, status)
                      : idft_aid<G2>(d_points, log_n, d_out, (hipStream_t)hip_stream, status);
}

int gwb_groth16_setup_ptau_phase_ms(float* ms) { return g_phases.read(ms); }

}  // extern "C"
