// A powers-of-tau ceremony on gfx950 (include/graph_witness_groth16_ceremony.h has the definitions): the batched point
// multiplication out[i] = s_i P_i with a scalar of its own per point, its scalars c tau'^(first + i), and the contribution to a
// `.ptau` that is built from the two, and the beacon, which is that contribution at the scalars of beacon.hpp.  Section 7, the transcript and the new file are ceremony.cc's (ceremony_internal.hpp);
// the conversion to affine bytes is setup.hip's, through its enqueue functions.
//
// mul_points_kernel<T, METHOD>, one point per thread.  METHOD 1 (plain) is fq_gfx950.hpp's xyzz_mul_short: with a scalar of its
// own in every lane a wave executes the conditional addition of nearly every bit.  METHOD 0 (windowed) recodes the scalar into
// signed digits of W bits and takes per window W doublings and at most one addition of a table entry:
//   * Recoding.  With N = ceil(254 / W) windows and C = sum_{j < N} 2^(W - 1) 2^(W j), the digit of window j is window j of
//     s + C minus 2^(W - 1).  That is the usual recoding from the bottom (d = window + carry; d >= 2^(W - 1) gives d - 2^W and a
//     carry) with its carries propagated by one 256-bit addition, so the digits can be taken from the top while the product is
//     formed.  Digits lie in [-2^(W - 1), 2^(W - 1) - 1], the top digit in [0, 2^(W - 1)]: r < 2^254 and r's bits from the top
//     window's lowest bit on are 3 (W = 3, 4: bits 252, 253) or 12 (W = 5: bits 250 to 253), so for s < r the top window is at most
//     that much plus a carry, which 2^(W - 1) holds: the carry never leaves the top window and s + C stays below 2^256.  The
//     static_assert of Window rests on exactly this.
//   * Table.  1 P .. 2^(W - 1) P per thread, as affine points: 1 P is the input and stays in registers; 2 P .. 2^(W - 1) P are made
//     in XYZZ and brought to affine form with one shared inversion per thread (1 / ZZ = (ZZ / ZZZ)^2, so the ZZZ alone are
//     inverted: about 400 Fq products, which the cheaper mixed addition of every window pays back).  They lie in LDS, word k of
//     entry e of lane l at dword (e words + k) 64 + l: the lane is the fastest index, so the 64 lanes of a ds_read_b32 hit 32 banks
//     twice over whatever entry each lane picks (MI355X: two lane groups of 32, bank = dword mod 32).  No runtime-indexed
//     per-thread array, no scratch: ZZ and ZZZ wait for the inversion in named registers, a choice between two points is made
//     limb by limb, and the inversion walks its exponent through one register.  A thread reads only what it wrote itself: no
//     barrier.  A negative digit negates y.
//   * Loop.  The top digit selects the first value of the accumulator (no addition).  A zero digit is skipped; while the
//     accumulator is the point at infinity its doublings are skipped, so leading zero windows cost nothing.
//   * Width: W = 3 in both groups, by measurement (profiles/ptau_contribute.txt has the final figures; 2^18 G1 and 2^17 G2 points,
//     random scalars, one MI355X, the aid's call with its conversion to affine).  The kernel runs at the speed its occupancy
//     allows, and LDS sets that.  With the table in XYZZ (128 B an entry in G1) W = 3 was 24 KB per wave, 6 waves per CU, 11.6 ms
//     against plain's 13.5 ms, and W = 4, 56 KB per wave, 2 waves per CU, 19.7 ms: less work and slower.  The affine table halves
//     an entry: W = 3 is 12 KB per wave in G1, so the registers bound it as they bound plain (3 waves per SIMD), 8.5 ms; in G2
//     24 KB per wave, one wave per SIMD by registers as everywhere in G2, 16.4 ms against plain's 29.0 ms (XYZZ table: 48 KB,
//     3 waves per CU, 25.2 ms).  W = 4 with affine entries would again be 28 KB per G1 wave, 5 waves per CU.
// The kernel also checks a point the way setup_ptau.hip's load_kernel does (coordinates, curve) when it is given a flag.
//
// fr_scalars_kernel: s_i = c tau'^(first + i), canonical, from the table tau'^(2^b) and c in device memory (not in the kernel
// arguments, which the caller could not zero).  It stands here and not beside contribute.hip's fr_powers_kernel so that the
// kernels of that file are compiled as before.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage for gfx950; every kernel: 0 bytes of scratch; VGPRs + AGPRs, LDS per
// workgroup of one wave, waves / SIMD by registers):
//   mul_points_kernel<G1, 0> 149, 12 KB, 3      mul_points_kernel<G1, 1> 144, no LDS, 3      fr_scalars_kernel 48, no LDS, 8
//   mul_points_kernel<G2, 0> 256 + 69, 24 KB, 1      mul_points_kernel<G2, 1> 256 + 46, no LDS, 1
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/graph_witness_groth16_beacon.h"
#include "../../include/graph_witness_groth16_ceremony.h"
#include "beacon.hpp"
#include "bn254_points_gfx950.hpp"
#include "ceremony_internal.hpp"
#include "contribute_internal.hpp"
#include "groth16_internal.hpp"
#include "ptau_internal.hpp"
#include "setup_internal.hpp"

using namespace cwc_r1cs;
using namespace cwc_g16;
using namespace cwc_contrib;
using namespace cwc_ceremony;
using cwc::Fr;

namespace {

constexpr uint32_t WAVE = 64;
constexpr unsigned long long NO_FAULT = ~0ull;

// ---- the windowed multiplication ---------------------------------------------------------------------------------------------

// The windows of a scalar below r for the width W (the header has the why).
template <uint32_t W>
struct Window {
    static_assert(W >= 3 && W <= 5, "a window of 3 to 5 bits");
    static constexpr uint32_t N = (254 + W - 1) / W;      // windows that cover the 254 bits of r
    static constexpr uint32_t TOP_SHIFT = W * (N - 1);     // the lowest bit of the top window
    static constexpr uint32_t TOP_BITS = 256 - TOP_SHIFT;  // the bits of s + C from there on
    static constexpr uint32_t HALF = 1u << (W - 1);
    static constexpr uint32_t ENTRIES = HALF - 1;          // 2 P .. HALF P in LDS, affine
    static_assert(TOP_SHIFT >= 224, "the top window lies in the scalar's last word");
    static_assert((CWC_P7 >> 30) == 0, "r < 2^254");
    // top window of s < r: at most r's, plus a carry; the top digit is that, and the window of s + C is HALF more
    static_assert((CWC_P7 >> (TOP_SHIFT - 224)) + 1 <= HALF, "the carry leaves the top window");
    static_assert(HALF + (CWC_P7 >> (TOP_SHIFT - 224)) + 1 < (1u << TOP_BITS), "s + C passes 2^256");
    // word i of C = sum_{j < N} HALF 2^(W j)
    static constexpr uint32_t offset_word(uint32_t i) {
        uint32_t w = 0;
        for (uint32_t j = 0; j < N; ++j) {
            const uint32_t bit = W * j + (W - 1);
            if (bit / 32 == i) w |= 1u << (bit % 32);
        }
        return w;
    }
};

template <class T>
constexpr uint32_t MUL_W = 3;  // per group; the header has the budget
// what a contribution multiplies with, per group: the faster of the two in profiles/ptau_contribute.txt
template <class T>
constexpr uint32_t MUL_DEFAULT = GWB_MUL_WINDOW;
template <class T>
constexpr uint32_t ENTRY_WORDS = sizeof(Affine<T>) / 4;  // a table entry is an affine point
template <class T>
constexpr size_t STORED_BYTES = sizeof(Affine<T>);

// x <<= S over the eight words (constant indices)
template <uint32_t S>
__device__ __forceinline__ void shl_words(Fr& x) {
#pragma unroll
    for (int i = 7; i > 0; --i) x.v[i] = (x.v[i] << S) | (x.v[i - 1] >> (32 - S));
    x.v[0] <<= S;
}

// One coordinate to and from a thread's column of the table: `col` is the LDS address of the thread's lane in dword 0, `at` the
// coordinate's first word.
__device__ __forceinline__ void lds_put(uint32_t* col, uint32_t at, const Fq& v) {
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) col[(at + k) * WAVE] = v.v[k];
}
__device__ __forceinline__ void lds_put(uint32_t* col, uint32_t at, const Fq2& v) {
    lds_put(col, at, v.c0);
    lds_put(col, at + 8, v.c1);
}
__device__ __forceinline__ void lds_get(const uint32_t* col, uint32_t at, Fq& v) {
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) v.v[k] = col[(at + k) * WAVE];
}
__device__ __forceinline__ void lds_get(const uint32_t* col, uint32_t at, Fq2& v) {
    lds_get(col, at, v.c0);
    lds_get(col, at + 8, v.c1);
}
// c ? a : b limb by limb (a choice between two whole points becomes a choice between their addresses, and both go to scratch)
__device__ __forceinline__ Fq pick(bool c, const Fq& a, const Fq& b) { return cwc::u256_select(c, a, b); }
__device__ __forceinline__ Fq2 pick(bool c, const Fq2& a, const Fq2& b) { return Fq2{pick(c, a.c0, b.c0), pick(c, a.c1, b.c1)}; }

// the affine point of entry `entry` of the thread's column
template <class T>
__device__ __forceinline__ void lds_put_entry(uint32_t* col, uint32_t entry, const typename T::E& x, const typename T::E& y) {
    constexpr uint32_t E = sizeof(typename T::E) / 4;
    lds_put(col, entry * ENTRY_WORDS<T>, x);
    lds_put(col, entry * ENTRY_WORDS<T> + E, y);
}
template <class T>
__device__ __forceinline__ Affine<T> lds_get_entry(const uint32_t* col, uint32_t entry) {
    constexpr uint32_t E = sizeof(typename T::E) / 4;
    Affine<T> q;
    lds_get(col, entry * ENTRY_WORDS<T>, q.x);
    lds_get(col, entry * ENTRY_WORDS<T> + E, q.y);
    return q;
}

// m P for m in [1, HALF]: P itself or the table's entry m - 2
template <class T>
__device__ __forceinline__ Affine<T> table_entry(const uint32_t* col, const Affine<T>& p, uint32_t m) {
    const Affine<T> q = lds_get_entry<T>(col, m >= 2 ? m - 2 : 0);
    return Affine<T>{pick(m == 1, p.x, q.x), pick(m == 1, p.y, q.y)};
}

// 1 / a = a^(q - 2), Montgomery in and out, 0 -> 0: fq_gfx950.hpp's fq_inv with the exponent's words moved up through one register
// (its table of eight words, indexed by the bit counter, is a per-thread array in scratch once it is inlined here)
__device__ __forceinline__ Fq inv_of(const Fq& a) {
    Fq e{{CWC_Q0 - 2u, CWC_Q1, CWC_Q2, CWC_Q3, CWC_Q4, CWC_Q5, CWC_Q6, CWC_Q7}};  // q0 > 2: no borrow
    Fq acc = fq_one();
#pragma unroll 1
    for (int w = 0; w < 8; ++w) {
        const uint32_t word = e.v[7];
#pragma unroll 1
        for (int b = 31; b >= 0; --b) {
            acc = fq_sqr(acc);
            if ((word >> b) & 1u) acc = fq_mul(acc, a);
        }
#pragma unroll
        for (int i = 7; i > 0; --i) e.v[i] = e.v[i - 1];
    }
    return acc;
}
__device__ __forceinline__ Fq2 inv_of(const Fq2& a) {  // (a0 - a1 u) / (a0^2 + a1^2)
    const Fq n = inv_of(fq_add(fq_sqr(a.c0), fq_sqr(a.c1)));
    return Fq2{fq_mul(a.c0, n), fq_neg(fq_mul(a.c1, n))};
}

// entry `entry` of the column, X and Y of a point with the given ZZ and 1 / ZZZ, becomes the affine point: x = X / ZZ with
// 1 / ZZ = (ZZ / ZZZ)^2, since ZZ^3 = ZZZ^2, and y = Y / ZZZ; a point at infinity (ZZ = 0) becomes (0, 0)
template <class T>
__device__ __forceinline__ void affine_entry(uint32_t* col, uint32_t entry, const typename T::E& zz, const typename T::E& inv_zzz) {
    Affine<T> q = lds_get_entry<T>(col, entry);
    const typename T::E r = T::mul(zz, inv_zzz);
    q.x = T::mul(q.x, T::sqr(r));
    q.y = T::mul(q.y, inv_zzz);
    const bool inf = T::is_zero(zz);
    lds_put_entry<T>(col, entry, pick(inf, T::zero(), q.x), pick(inf, T::zero(), q.y));
}

// s a for a canonical s < r and a point a that is not the point at infinity; `col` as above, ENTRIES affine points of room
template <class T, uint32_t W>
__device__ __forceinline__ Xyzz<T> xyzz_mul_window(const Affine<T>& a, const Fr& s, uint32_t* col) {
    using Win = Window<W>;
    using E = typename T::E;
    static_assert(Win::ENTRIES == 3, "the shared inversion below is written out for the three entries of W = 3");
    // 2 P, 3 P, 4 P: X and Y go to the table as they come, ZZ and ZZZ stay in named registers (an array indexed in a loop would
    // go to scratch) for one shared inversion; 1 takes the place of the ZZZ of an entry at infinity
    Xyzz<T> t = xyzz_dbl(Xyzz<T>{a.x, a.y, T::one(), T::one()});
    lds_put_entry<T>(col, 0, t.X, t.Y);
    const E zz0 = t.ZZ, z0 = T::is_zero(t.ZZZ) ? T::one() : t.ZZZ;
    t = xyzz_add_affine(t, a);
    lds_put_entry<T>(col, 1, t.X, t.Y);
    const E zz1 = t.ZZ, z1 = T::is_zero(t.ZZZ) ? T::one() : t.ZZZ;
    t = xyzz_add_affine(t, a);
    lds_put_entry<T>(col, 2, t.X, t.Y);
    const E zz2 = t.ZZ, z2 = T::is_zero(t.ZZZ) ? T::one() : t.ZZZ;
    const E z01 = T::mul(z0, z1);
    E inv = inv_of(T::mul(z01, z2));
    affine_entry<T>(col, 2, zz2, T::mul(inv, z01));
    inv = T::mul(inv, z2);  // 1 / (ZZZ_0 ZZZ_1)
    affine_entry<T>(col, 1, zz1, T::mul(inv, z0));
    affine_entry<T>(col, 0, zz0, T::mul(inv, z1));
    Fr k;
    cwc::u256_add(k, s, Fr{{Win::offset_word(0), Win::offset_word(1), Win::offset_word(2), Win::offset_word(3), Win::offset_word(4), Win::offset_word(5),
                            Win::offset_word(6), Win::offset_word(7)}});
    // in [0, HALF] for s < r; the bound keeps a scalar that is not inside the table all the same
    const uint32_t top = min((k.v[7] >> (32 - Win::TOP_BITS)) - Win::HALF, Win::HALF);
    shl_words<Win::TOP_BITS>(k);
    const Affine<T> first = table_entry<T>(col, a, top);
    Xyzz<T> acc = top == 0 ? xyzz_inf<T>() : from_affine(first);
#pragma unroll 1
    for (uint32_t j = 1; j < Win::N; ++j) {
        if (!xyzz_is_inf(acc)) {
#pragma unroll 1
            for (uint32_t b = 0; b < W; ++b) acc = xyzz_dbl(acc);
        }
        const int32_t d = (int32_t)(k.v[7] >> (32 - W)) - (int32_t)Win::HALF;
        shl_words<W>(k);
        if (d != 0) {
            Affine<T> q = table_entry<T>(col, a, (uint32_t)(d < 0 ? -d : d));
            if (d < 0) q.y = T::neg(q.y);
            if (!affine_is_inf(q)) acc = xyzz_add_affine(acc, q);
        }
    }
    return acc;
}

// out[i] = scalars[i] in[i] for the stored points in[0 .. n) (Montgomery, or canonical; zero bytes: infinity, which stays) and
// canonical scalars below r, XYZZ.  flag != nullptr: the point is checked, and the smallest 2 i + fault of the array is left in
// *flag (setup_ptau.hip's load_kernel); a refused point gives infinity.  A workgroup is one wave.
template <class T, uint32_t METHOD>
__global__ __launch_bounds__(WAVE) void mul_points_kernel(const uint8_t* __restrict__ in, const Fr* __restrict__ scalars, uint32_t n, uint32_t canonical,
                                                          Xyzz<T>* __restrict__ out, unsigned long long* __restrict__ flag) {
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n) return;
    Affine<T> a;
    const bool in_range = get_coords<T>(in + (size_t)i * STORED_BYTES<T>, canonical != 0, a.x, a.y);
    bool inf = affine_is_inf(a);
    if (flag) {
        if (!in_range) {
            atomicMin(flag, 2ull * i + (uint32_t)PointFault::COORDINATE);
            inf = true;
        } else if (!inf && !on_curve(a, curve_b<T>())) {
            atomicMin(flag, 2ull * i + (uint32_t)PointFault::CURVE);
            inf = true;
        }
    }
    if (inf) {
        out[i] = xyzz_inf<T>();
        return;
    }
    const Fr s = scalars[i];
    if constexpr (METHOD == 1) {
        out[i] = xyzz_mul_short(Xyzz<T>{a.x, a.y, T::one(), T::one()}, s);
    } else {
        __shared__ uint32_t table[Window<MUL_W<T>>::ENTRIES * ENTRY_WORDS<T> * WAVE];
        out[i] = xyzz_mul_window<T, MUL_W<T>>(a, s, table + threadIdx.x);
    }
}

// out[k] = c tau^(first + k), canonical, for k < count; tab: tau^(2^b) for b < POW_BITS, then c, Montgomery form
__global__ __launch_bounds__(256) void fr_scalars_kernel(Fr* __restrict__ out, uint32_t count, uint64_t first, const Fr* __restrict__ tab) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const uint64_t e = first + k;
    Fr x = tab[POW_BITS];
    for (uint32_t b = 0; b < POW_BITS; ++b)
        if ((e >> b) & 1u) x = cwc::fr_mul(x, tab[b]);
    out[k] = cwc::fr_from_mont(x);
}

// ---- host -----------------------------------------------------------------------------------------------------------------

template <class T>
void enqueue_mul(const uint8_t* d_in, const Fr* d_scalars, uint32_t n, bool canonical, uint32_t method, Xyzz<T>* d_out, unsigned long long* d_flag,
                 hipStream_t s) {
    const dim3 grid(blocks_for(n, WAVE)), block(WAVE);
    if (method == GWB_MUL_PLAIN)
        hipLaunchKernelGGL((mul_points_kernel<T, 1>), grid, block, 0, s, d_in, d_scalars, n, canonical ? 1u : 0u, d_out, d_flag);
    else
        hipLaunchKernelGGL((mul_points_kernel<T, 0>), grid, block, 0, s, d_in, d_scalars, n, canonical ? 1u : 0u, d_out, d_flag);
}

template <class T>
void enqueue_affine(const void* d_xyzz, uint32_t n, uint8_t* d_out, bool canonical, hipStream_t s) {
    if constexpr (std::is_same<T, G1>::value)
        cwc_setup::enqueue_affine_g1(d_xyzz, n, d_out, canonical, s);
    else
        cwc_setup::enqueue_affine_g2(d_xyzz, n, d_out, canonical, s);
}

// the aid of mul_points_kernel for one group (the extern functions below)
template <class T>
int mul_aid(const char* fn, const void* d_points, const void* d_scalars, size_t n, uint32_t form, uint32_t method, void* d_out, void* hip_stream,
            gw_status_t* status) {
    if (form != GWB_FORM_CANONICAL && form != GWB_FORM_MONTGOMERY) return fail(status, std::string(fn) + ": unknown form " + std::to_string(form));
    if (method != GWB_MUL_WINDOW && method != GWB_MUL_PLAIN) return fail(status, std::string(fn) + ": unknown method " + std::to_string(method));
    if (n && (!d_points || !d_scalars || !d_out)) return fail(status, std::string(fn) + ": NULL argument");
    if (n > 0x7fffffffull) return fail(status, std::string(fn) + ": n above 2^31 - 1");
    if (n == 0) {
        set_ok(status);
        return 0;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    void* ws = nullptr;
    hipError_t e = hipMallocAsync(&ws, n * sizeof(Xyzz<T>), s);
    if (e != hipSuccess) return fail(status, hip_err("allocating the multiplication's workspace", e));
    const bool canonical = form == GWB_FORM_CANONICAL;
    enqueue_mul<T>((const uint8_t*)d_points, (const Fr*)d_scalars, (uint32_t)n, canonical, method, (Xyzz<T>*)ws, nullptr, s);
    enqueue_affine<T>(ws, (uint32_t)n, (uint8_t*)d_out, canonical, s);
    e = hipGetLastError();
    const hipError_t ef = hipFreeAsync(ws, s);
    if (e != hipSuccess) return fail(status, hip_err("launching the multiplication", e));
    if (ef != hipSuccess) return fail(status, hip_err("releasing the multiplication's workspace", ef));
    set_ok(status);
    return 0;
}

// ---- the contribution -------------------------------------------------------------------------------------------------------

PhaseTimes<5> g_phases;  // load, scalars, mul_g1, mul_g2, affine: summed over the pieces

// What a contribution keeps on the device: the stream, the events around a piece's phases, the workspace, and `secret`: the
// tables of the three scalar families and the piece's scalars, zeroed by ~SetupDevice before they are released.
using CeremonyDevice = SetupDevice<5>;

// out = (c tau'^(first + i)) in[i] over the n stored points of one section, in pieces; d_tab: the family's table on the device.
// A point fault goes to err in point_message's words.
template <class T>
bool contribute_section(uint32_t id, const uint8_t* in, uint64_t n, const Fr* d_tab, CeremonyDevice& D, uint64_t chunk, size_t o_scalars, uint8_t* out,
                        float (&ms)[5], bool& timed, std::string& err) {
    constexpr bool g2 = !std::is_same<T, G1>::value;
    constexpr size_t PB = STORED_BYTES<T>;
    uint8_t* W = D.work.as<uint8_t>();
    Carve cw;
    const size_t o_in = cw.take(chunk * G2_BYTES), o_x = cw.take(chunk * sizeof(Xyzz<G2>)), o_out = cw.take(chunk * G2_BYTES), o_flag = cw.take(8);
    Fr* d_scalars = (Fr*)(D.secret.as<uint8_t>() + o_scalars);
    unsigned long long* d_flag = (unsigned long long*)(W + o_flag);
    for (uint64_t at = 0; at < n; at += chunk) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - at);
        unsigned long long fault = NO_FAULT;
        D.ev.record(0, D.s);
        hipError_t e = hipMemcpyAsync(W + o_in, in + at * PB, (size_t)m * PB, hipMemcpyHostToDevice, D.s);
        if (e == hipSuccess) e = hipMemsetAsync(d_flag, 0xff, 8, D.s);
        if (e != hipSuccess) {
            err = hip_err("uploading a piece of ceremony points", e);
            return false;
        }
        D.ev.record(1, D.s);
        hipLaunchKernelGGL(fr_scalars_kernel, dim3(blocks_for(m, 256)), dim3(256), 0, D.s, d_scalars, m, at, d_tab);
        D.ev.record(2, D.s);
        enqueue_mul<T>(W + o_in, d_scalars, m, false, MUL_DEFAULT<T>, (Xyzz<T>*)(W + o_x), d_flag, D.s);
        D.ev.record(3, D.s);
        enqueue_affine<T>(W + o_x, m, W + o_out, false, D.s);
        D.ev.record(4, D.s);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out + at * PB, W + o_out, (size_t)m * PB, hipMemcpyDeviceToHost, D.s);
        if (e == hipSuccess) e = hipMemcpyAsync(&fault, d_flag, 8, hipMemcpyDeviceToHost, D.s);
        if (e == hipSuccess) e = hipStreamSynchronize(D.s);  // the piece's buffers are written again by the next piece
        if (e != hipSuccess) {
            err = hip_err("multiplying a piece of ceremony points", e);
            return false;
        }
        if (fault != NO_FAULT) {
            err = cwc_ptau::point_message(id, at + (fault >> 1), (PointFault)(fault & 1), g2);
            return false;
        }
        float t[4];
        if (D.ev.elapsed(t) == hipSuccess) {
            ms[0] += t[0];
            ms[1] += t[1];
            ms[g2 ? 3 : 2] += t[2];
            ms[4] += t[3];
        } else {
            timed = false;
        }
    }
    return true;
}

// the three secrets of a contribution and what derives from them on the host; zeroed when it goes
struct Secrets {
    Fr x[3];              // tau', alpha', beta', canonical
    Fr nonce[3];          // the s of the three keys
    Fr tab[3][POW_BITS + 1];  // per family tau'^(2^b), then the factor: 1, alpha', beta'; Montgomery form
    ~Secrets() { explicit_bzero(this, sizeof *this); }
};

bool draw_nonzero(Fr& x, std::string& err) {
    do {
        if (!draw_fr(x, err)) return false;
    } while (cwc::u256_is_zero(x));
    return true;
}

// The file and its section 7 as a contribution or a beacon reads them, before the device is touched; 0, or 2 with the message.
int read_input(const uint8_t* ptau, size_t len, cwc_ptau::View& view, Section7& s7, gw_status_t* status) {
    std::string err;
    if (!cwc_ptau::parse(ptau, len, view, err) || !parse_section7(view.sec[7].p, view.sec[7].size, s7, err)) return fail2(status, err);
    if (point_fault<G2>(view.sec[6].p, false) != PointFault::NONE)
        return fail2(status, cwc_ptau::point_message(6, 0, point_fault<G2>(view.sec[6].p, false), true));
    return 0;
}

// The one path of a contribution and of a beacon: the secrets sec.x and the nonces sec.nonce, both in [1, r), are applied to the
// parsed file, and the record of the given type with the given parameters is appended.
int apply(const cwc_ptau::View& view, Section7& s7, Secrets& sec, uint32_t type, const std::vector<uint8_t>& params, const std::string& nm, void** out,
          size_t* out_len, uint8_t* hash64, gw_status_t* status) {
    std::string err;
    for (int j = 0; j < 3; ++j) {
        sec.tab[j][0] = cwc::fr_to_mont(sec.x[0]);
        for (uint32_t b = 1; b < POW_BITS; ++b) sec.tab[j][b] = cwc::fr_mul(sec.tab[j][b - 1], sec.tab[j][b - 1]);
        sec.tab[j][POW_BITS] = j ? cwc::fr_to_mont(sec.x[j]) : cwc::fr_one();
    }

    // the new file's sections 2 to 6, sized before the device is touched
    const uint64_t np = 1ull << view.power, n_t1 = 2 * np - 1;
    std::vector<uint8_t> t1(n_t1 * G1_BYTES), t2(np * G2_BYTES), at(np * G1_BYTES), bt(np * G1_BYTES);
    uint8_t beta2[G2_BYTES];
    {
        CeremonyDevice D;
        const uint64_t chunk = std::max<uint64_t>(1, std::min(piece_points("CWC_CONTRIBUTE_CHUNK"), n_t1));
        Carve cw, cs;
        cw.take(chunk * G2_BYTES);
        cw.take(chunk * sizeof(Xyzz<G2>));
        cw.take(chunk * G2_BYTES);
        cw.take(8);
        const size_t o_tab = cs.take(sizeof sec.tab), o_scalars = cs.take(chunk * sizeof(Fr));
        hipError_t e = D.open(cs.o, cw.o);
        if (e != hipSuccess) return fail2(status, hip_err("allocating the contribution's workspace", e));
        e = hipMemcpyAsync(D.secret.as<uint8_t>() + o_tab, sec.tab, sizeof sec.tab, hipMemcpyHostToDevice, D.s);
        if (e == hipSuccess) e = hipStreamSynchronize(D.s);  // the copy has left the host table
        if (e != hipSuccess) return fail2(status, hip_err("uploading the contribution's scalars", e));
        const Fr* d_tab = (const Fr*)(D.secret.as<uint8_t>() + o_tab);
        float ms[5] = {0, 0, 0, 0, 0};
        bool timed = true;
        if (!contribute_section<G1>(2, view.sec[2].p, n_t1, d_tab, D, chunk, o_scalars, t1.data(), ms, timed, err) ||
            !contribute_section<G2>(3, view.sec[3].p, np, d_tab, D, chunk, o_scalars, t2.data(), ms, timed, err) ||
            !contribute_section<G1>(4, view.sec[4].p, np, d_tab + (POW_BITS + 1), D, chunk, o_scalars, at.data(), ms, timed, err) ||
            !contribute_section<G1>(5, view.sec[5].p, np, d_tab + 2 * (POW_BITS + 1), D, chunk, o_scalars, bt.data(), ms, timed, err))
            return fail2(status, err);
        e = hipMemsetAsync(D.secret.as(), 0, D.secret_bytes, D.s);
        if (e == hipSuccess) e = hipStreamSynchronize(D.s);
        if (e != hipSuccess) return fail2(status, hip_err("clearing the contribution's scalars", e));
        g_phases.store(ms, timed);
    }
    g2_mul_stored(view.sec[6].p, sec.x[2], beta2);

    // the record: the after-values, then per secret the key against the challenge before this record
    PtauRecord rec;
    memcpy(rec.tau_g1, t1.data() + G1_BYTES, G1_BYTES);
    memcpy(rec.tau_g2, t2.data() + G2_BYTES, G2_BYTES);
    memcpy(rec.alpha_g1, at.data(), G1_BYTES);
    memcpy(rec.beta_g1, bt.data(), G1_BYTES);
    memcpy(rec.beta_g2, beta2, G2_BYTES);
    uint8_t challenge[HASH_BYTES], gen1[G1_BYTES];
    last_challenge(view.sec[1].p, view.sec[1].size, s7, s7.recs.size(), challenge);
    put_stored(gen1, g1_generator());
    for (uint32_t j = 0; j < 3; ++j) {
        uint8_t sp[G2_BYTES];
        g1_mul_stored(gen1, sec.nonce[j], rec.g1_s[j]);
        g1_mul_stored(rec.g1_s[j], sec.x[j], rec.g1_sx[j]);
        put_stored(sp, key_challenge_point(challenge, j, rec.g1_s[j], rec.g1_sx[j]));
        g2_mul_stored(sp, sec.x[j], rec.g2_spx[j]);
    }
    rec.type = type;
    rec.params = params;
    rec.name = nm;
    next_challenge(challenge, rec, rec.next_challenge);
    memcpy(hash64, rec.next_challenge, HASH_BYTES);
    s7.recs.push_back(rec);

    const uint8_t* bodies[5] = {t1.data(), t2.data(), at.data(), bt.data(), beta2};
    return write_contributed(view, bodies, s7, out, out_len, status);
}

int contribute(const uint8_t* ptau, size_t len, const char* name, const uint8_t* secrets96, void** out, size_t* out_len, uint8_t* hash64, gw_status_t* status) {
    std::string err;
    cwc_ptau::View view;
    Section7 s7;
    if (read_input(ptau, len, view, s7, status) != 0) return 2;
    const std::string nm = name ? name : "";
    if (nm.size() > GWB_CONTRIBUTION_NAME_MAX) return fail2(status, "ptau contribute: the name has " + std::to_string(nm.size()) + " bytes, 255 at the most");
    Secrets sec;
    static const char* which[3] = {"tau", "alpha", "beta"};
    for (int j = 0; j < 3; ++j) {
        if (secrets96) {
            memcpy(sec.x[j].v, secrets96 + 32 * j, 32);
            if (cwc::u256_is_zero(sec.x[j]) || !cwc::u256_lt(sec.x[j], cwc::fr_p()))
                return fail2(status, std::string("ptau contribute: the secret ") + which[j] + " is not in [1, r)");
        } else if (!draw_nonzero(sec.x[j], err)) {
            return fail2(status, err);
        }
        if (!draw_nonzero(sec.nonce[j], err)) return fail2(status, err);
    }
    return apply(view, s7, sec, 0, name_params(nm), nm, out, out_len, hash64, status);
}

// A beacon is the contribution whose secrets and nonces its parameters give (beacon.hpp); they are public, so that the zeroing
// of `Secrets` protects nothing here.
int beacon(const uint8_t* ptau, size_t len, const char* name, const uint8_t* hash, size_t hash_len, uint32_t exp, void** out, size_t* out_len, uint8_t* hash64,
           gw_status_t* status) {
    const std::string nm = name ? name : "";
    const std::string fault = cwc_beacon::argument_fault(nm.size(), hash_len, exp, cwc_beacon::limit());
    if (!fault.empty()) return fail2(status, fault);
    cwc_ptau::View view;
    Section7 s7;
    if (read_input(ptau, len, view, s7, status) != 0) return 2;
    Fr derived[cwc_beacon::PHASE1_SCALARS];
    cwc_beacon::scalars(1, hash, hash_len, exp, derived);
    Secrets sec;
    for (int j = 0; j < 3; ++j) {
        sec.x[j] = derived[j];
        sec.nonce[j] = derived[3 + j];
    }
    return apply(view, s7, sec, 1, cwc_beacon::write_params(nm, exp, hash, hash_len), nm, out, out_len, hash64, status);
}

// ---- verification -------------------------------------------------------------------------------------------------------------

bool is_zero_bytes(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (p[i]) return false;
    return true;
}

// the five points that a record's after-values continue or equal: of a file, or the generators
struct Anchors {
    const uint8_t *tau_g1, *tau_g2, *alpha_g1, *beta_g1, *beta_g2;
};
Anchors anchors_of(const cwc_ptau::View& v) {
    return {v.sec[2].p + G1_BYTES, v.sec[3].p + G2_BYTES, v.sec[4].p, v.sec[5].p, v.sec[6].p};
}
Anchors anchors_of(const PtauRecord& r) { return {r.tau_g1, r.tau_g2, r.alpha_g1, r.beta_g1, r.beta_g2}; }

struct Generators {
    uint8_t g1[G1_BYTES], g2[G2_BYTES];
    Generators() {
        put_stored(g1, g1_generator());
        put_stored(g2, g2_generator());
    }
    Anchors anchors() const { return {g1, g2, g1, g1, g2}; }
};

// The rules of record k (0-based) of s against the challenge before it and the points before it; "" or what fails on the host.
// The record's eight pairing rules go to `checks`; sp (three stored G2 points) gets the challenge points and has to outlive
// the checks, as `gen` has.
std::string record_rules(const Section7& s, size_t k, const uint8_t challenge[HASH_BYTES], const Anchors& prev, const Generators& gen, uint8_t* sp,
                         std::vector<PairCheck>& checks) {
    const PtauRecord& r = s.recs[k];
    const std::string who = "ptau: contribution " + std::to_string(k + 1) + ": ";
    static const char* secret[3] = {"tau", "alpha", "beta"};
    uint8_t t[HASH_BYTES];
    next_challenge(challenge, r, t);
    if (memcmp(t, r.next_challenge, HASH_BYTES) != 0) return who + "nextChallenge is not that of the challenge before the record and the record's points";
    const struct {
        std::string name;
        const uint8_t* at;
        size_t bytes;
    } pts[14] = {{"tauG1", r.tau_g1, G1_BYTES},          {"tauG2", r.tau_g2, G2_BYTES},          {"alphaG1", r.alpha_g1, G1_BYTES},
                 {"betaG1", r.beta_g1, G1_BYTES},        {"betaG2", r.beta_g2, G2_BYTES},        {"tau_g1_s", r.g1_s[0], G1_BYTES},
                 {"tau_g1_sx", r.g1_sx[0], G1_BYTES},    {"alpha_g1_s", r.g1_s[1], G1_BYTES},    {"alpha_g1_sx", r.g1_sx[1], G1_BYTES},
                 {"beta_g1_s", r.g1_s[2], G1_BYTES},     {"beta_g1_sx", r.g1_sx[2], G1_BYTES},   {"tau_g2_spx", r.g2_spx[0], G2_BYTES},
                 {"alpha_g2_spx", r.g2_spx[1], G2_BYTES}, {"beta_g2_spx", r.g2_spx[2], G2_BYTES}};
    for (const auto& p : pts)
        if (is_zero_bytes(p.at, p.bytes)) return who + p.name + " is the point at infinity";
    for (int j = 0; j < 3; ++j)
        if (!g2_stored_in_subgroup(r.g2_spx[j])) return who + secret[j] + "_g2_spx is not in the order-r subgroup of G2";
    if (!g2_stored_in_subgroup(r.tau_g2)) return who + "tauG2 is not in the order-r subgroup of G2";
    if (!g2_stored_in_subgroup(r.beta_g2)) return who + "betaG2 is not in the order-r subgroup of G2";
    for (uint32_t j = 0; j < 3; ++j) {
        put_stored(sp + j * G2_BYTES, key_challenge_point(challenge, j, r.g1_s[j], r.g1_sx[j]));
        checks.push_back({r.g1_s[j], r.g2_spx[j], r.g1_sx[j], sp + j * G2_BYTES,
                          who + secret[j] + "_g1_sx is not " + secret[j] + "_g1_s times the secret that " + secret[j] + "_g2_spx proves"});
    }
    const uint8_t *after[3] = {r.tau_g1, r.alpha_g1, r.beta_g1}, *before[3] = {prev.tau_g1, prev.alpha_g1, prev.beta_g1};
    for (uint32_t j = 0; j < 3; ++j)
        checks.push_back({after[j], sp + j * G2_BYTES, before[j], r.g2_spx[j],
                          who + secret[j] + "G1 is not the previous " + secret[j] + "G1 times the proven secret"});
    checks.push_back({r.tau_g1, gen.g2, gen.g1, r.tau_g2, who + "tauG2 is not the G2 generator times tauG1's scalar"});
    checks.push_back({r.beta_g1, gen.g2, gen.g1, r.beta_g2, who + "betaG2 is not the G2 generator times betaG1's scalar"});
    if (r.type == 1) {  // the beacon rule: the keys' G1 points are those of the derived secrets and nonces; the pairings above fix the rest
        const cwc_beacon::Form f = cwc_beacon::form_of(r.params, cwc_beacon::MAX_EXP);  // form and limit were checked before the device
        if (f.rc != 0) return who + f.msg;
        Fr derived[cwc_beacon::PHASE1_SCALARS];
        cwc_beacon::scalars(1, f.items.hash, f.items.hash_len, f.items.exp, derived);
        for (uint32_t j = 0; j < 3; ++j) {
            uint8_t g1_s[G1_BYTES], g1_sx[G1_BYTES];
            g1_mul_stored(gen.g1, derived[3 + j], g1_s);
            g1_mul_stored(g1_s, derived[j], g1_sx);
            if (memcmp(g1_s, r.g1_s[j], G1_BYTES) != 0 || memcmp(g1_sx, r.g1_sx[j], G1_BYTES) != 0)
                return who + "the key of secret " + secret[j] + " is not the one its beaconHash and numIterationsExp give";
        }
    }
    return "";
}

// the after-values `a` (of the last record, or the generators) are the file's points; "" or which is not
std::string anchors_rule(const Anchors& a, const cwc_ptau::View& v, const std::string& whose) {
    const Anchors f = anchors_of(v);
    const struct {
        const char* name;
        const uint8_t *want, *have;
        size_t bytes;
    } pts[5] = {{"tauG1[1]", a.tau_g1, f.tau_g1, G1_BYTES},
                {"tauG2[1]", a.tau_g2, f.tau_g2, G2_BYTES},
                {"alphaTauG1[0]", a.alpha_g1, f.alpha_g1, G1_BYTES},
                {"betaTauG1[0]", a.beta_g1, f.beta_g1, G1_BYTES},
                {"betaG2", a.beta_g2, f.beta_g2, G2_BYTES}};
    for (const auto& p : pts)
        if (memcmp(p.want, p.have, p.bytes) != 0) return std::string("ptau: ") + p.name + " of the file is not " + whose;
    return "";
}

// rc and message of a verification
struct Outcome {
    int rc = 0;
    std::string msg;
};

// Rule 3, the whole-file powers check, after the rules that left host_verdict and `checks`, and then every pairing in one
// launch.  The first rule that fails is the verdict: a pairing rule collected before the host rule that stopped the collection.
Outcome finish_verification(const cwc_ptau::View& view, const uint8_t* seed_in, std::string host_verdict, std::vector<PairCheck>& checks) {
    std::string err, verdict;
    PowersSums sums;
    if (host_verdict.empty()) {
        const uint64_t np = 1ull << view.power;
        const int rc = cwc_ptau::check_g2_points(3, 0, view.sec[3].p, np, err);
        if (rc == 2) return {2, err};
        if (rc == 1) host_verdict = err;
        uint8_t seed[32];
        if (host_verdict.empty()) {
            if (!seed_or_draw(seed_in, seed)) return {2, "ptau: getrandom failed"};  // drawn after the file is seen
            cwc_ptau::Plan pl;
            pl.p = view.power;
            pl.t1 = view.sec[2].p;
            pl.t2 = view.sec[3].p;
            pl.at = view.sec[4].p;
            pl.bt = view.sec[5].p;
            pl.beta2 = view.sec[6].p;
            if (!powers_rules(pl, np, 2 * np - 2, true, seed, sums, checks, host_verdict, err)) return {2, err};
        }
    }
    if (!run_pair_checks(checks, verdict, err)) return {2, err};
    if (verdict.empty()) verdict = host_verdict;
    return {verdict.empty() ? 0 : 1, verdict};
}

Outcome verify(const uint8_t* ptau, size_t len, uint32_t flags, const uint8_t* seed_in, uint8_t* hashes_out, size_t* n_io) {
    std::string err;
    cwc_ptau::View view;
    Section7 s7;
    if (!cwc_ptau::parse(ptau, len, view, err) || !parse_section7(view.sec[7].p, view.sec[7].size, s7, err) || !cwc_ptau::check_all_points(view, err))
        return {2, err};
    if (!(flags & GWB_PTAU_VERIFY_SKIP_RECORDS)) {
        const int rc = cwc_beacon::forms_of(s7.recs, 0, "ptau", err);
        if (rc != 0) return {rc, err};
    }
    const size_t n = s7.recs.size();
    const Generators gen;
    std::vector<PairCheck> checks;
    std::vector<uint8_t> sp(std::max<size_t>(n, 1) * 3 * G2_BYTES);
    std::string host_verdict;
    if (!(flags & GWB_PTAU_VERIFY_SKIP_RECORDS)) {
        uint8_t challenge[HASH_BYTES];
        for (size_t k = 0; k < n && host_verdict.empty(); ++k) {
            last_challenge(view.sec[1].p, view.sec[1].size, s7, k, challenge);  // the one before was found as recomputed
            host_verdict = record_rules(s7, k, challenge, k ? anchors_of(s7.recs[k - 1]) : gen.anchors(), gen, sp.data() + k * 3 * G2_BYTES, checks);
        }
        if (host_verdict.empty())
            host_verdict = n ? anchors_rule(anchors_of(s7.recs[n - 1]), view, "the after-value of the last contribution")
                             : anchors_rule(gen.anchors(), view, "the generator, and no contribution accounts for it");
    }
    const Outcome o = finish_verification(view, seed_in, host_verdict, checks);
    if (o.rc != 0) return o;
    const size_t room = *n_io;
    *n_io = n;
    for (size_t k = 0; k < n && k < room && hashes_out; ++k) memcpy(hashes_out + k * HASH_BYTES, s7.recs[k].next_challenge, HASH_BYTES);
    return o;
}

Outcome verify_step(const uint8_t* prev_bytes, size_t prev_len, const uint8_t* next_bytes, size_t next_len, const uint8_t* seed_in) {
    std::string err;
    cwc_ptau::View prev, next;
    Section7 sa, sb;
    if (!cwc_ptau::parse(prev_bytes, prev_len, prev, err) || !parse_section7(prev.sec[7].p, prev.sec[7].size, sa, err)) return {2, "previous file: " + err};
    if (!cwc_ptau::parse(next_bytes, next_len, next, err) || !parse_section7(next.sec[7].p, next.sec[7].size, sb, err) || !cwc_ptau::check_all_points(next, err))
        return {2, "next file: " + err};
    if (prev.sec[1].size != next.sec[1].size || memcmp(prev.sec[1].p, next.sec[1].p, prev.sec[1].size) != 0)
        return {1, "ptau step: section 1 (header) differs from the previous file's"};
    if (sb.recs.size() != sa.recs.size() + 1)
        return {1, "ptau step: section 7 of the next file has " + std::to_string(sb.recs.size()) + " contributions, the previous file " +
                       std::to_string(sa.recs.size()) + ": exactly one more is expected"};
    if (!sa.recs.empty()) {  // records lie one after the other: the earlier ones are a prefix of the section's bytes
        const size_t prefix = (size_t)prev.sec[7].size - 4;
        if (memcmp(prev.sec[7].p + 4, next.sec[7].p + 4, prefix) != 0) {
            size_t k = 0;
            std::vector<uint8_t> a, b;
            for (; k + 1 < sa.recs.size(); ++k) {
                a.clear();
                b.clear();
                write_section7(Section7{{sa.recs[k]}}, a);
                write_section7(Section7{{sb.recs[k]}}, b);
                if (a != b) break;
            }
            return {1, "ptau step: section 7: contribution " + std::to_string(k + 1) + " is not the previous file's"};
        }
    }
    if (const int rc = cwc_beacon::forms_of(sb.recs, sb.recs.size() - 1, "ptau", err)) return {rc, err};  // the new record, if it is a beacon
    const Anchors before = anchors_of(prev);
    const struct {
        const char* name;
        const uint8_t* at;
        bool g2;
    } pts[5] = {{"tauG1[1]", before.tau_g1, false}, {"tauG2[1]", before.tau_g2, true}, {"alphaTauG1[0]", before.alpha_g1, false},
                {"betaTauG1[0]", before.beta_g1, false}, {"betaG2", before.beta_g2, true}};
    for (const auto& p : pts) {
        const PointFault f = p.g2 ? point_fault<G2>(p.at, false) : point_fault<G1>(p.at, false);
        if (f != PointFault::NONE) return {2, std::string("previous file: ptau: ") + p.name + (f == PointFault::CURVE ? " is not on its curve" : " has a coordinate >= q")};
        if (is_zero_bytes(p.at, p.g2 ? G2_BYTES : G1_BYTES)) return {1, std::string("ptau step: ") + p.name + " of the previous file is the point at infinity"};
    }
    const Generators gen;
    std::vector<PairCheck> checks;
    uint8_t sp[3 * G2_BYTES], challenge[HASH_BYTES];
    const size_t k = sb.recs.size() - 1;
    last_challenge(prev.sec[1].p, prev.sec[1].size, sa, k, challenge);
    std::string host_verdict = record_rules(sb, k, challenge, before, gen, sp, checks);
    if (host_verdict.empty()) host_verdict = anchors_rule(anchors_of(sb.recs[k]), next, "the after-value of the new contribution");
    return finish_verification(next, seed_in, host_verdict, checks);
}

int finish(const Outcome& o, gw_status_t* status) {
    if (o.rc == 0) {
        set_ok(status);
        return 0;
    }
    set_status(status, o.msg);
    return o.rc;
}

}  // namespace

extern "C" {

int gwb_ptau_verify(const void* ptau, size_t len, uint32_t flags, const uint8_t* seed, void* hashes_out, size_t* n, gw_status_t* status) {
    if (!n || (!ptau && len) || (*n && !hashes_out)) return fail2(status, "gwb_ptau_verify: NULL argument");
    if (flags & ~(uint32_t)GWB_PTAU_VERIFY_SKIP_RECORDS) return fail2(status, "gwb_ptau_verify: unknown flags " + std::to_string(flags));
    try {
        return finish(verify((const uint8_t*)ptau, len, flags, seed, (uint8_t*)hashes_out, n), status);
    } catch (const std::bad_alloc&) {
        return fail2(status, "ptau: out of host memory");
    }
}

int gwb_ptau_verify_step(const void* prev, size_t prev_len, const void* next, size_t next_len, const uint8_t* seed, gw_status_t* status) {
    if ((!prev && prev_len) || (!next && next_len)) return fail2(status, "gwb_ptau_verify_step: NULL argument");
    try {
        return finish(verify_step((const uint8_t*)prev, prev_len, (const uint8_t*)next, next_len, seed), status);
    } catch (const std::bad_alloc&) {
        return fail2(status, "ptau: out of host memory");
    }
}

int gwb_bn254_g1_mul_batch_device(const void* d_points, const void* d_scalars, size_t n, uint32_t form, uint32_t method, void* d_out, void* hip_stream,
                                  gw_status_t* status) {
    return mul_aid<G1>("gwb_bn254_g1_mul_batch_device", d_points, d_scalars, n, form, method, d_out, hip_stream, status);
}

int gwb_bn254_g2_mul_batch_device(const void* d_points, const void* d_scalars, size_t n, uint32_t form, uint32_t method, void* d_out, void* hip_stream,
                                  gw_status_t* status) {
    return mul_aid<G2>("gwb_bn254_g2_mul_batch_device", d_points, d_scalars, n, form, method, d_out, hip_stream, status);
}

int gwb_ptau_contribute(const void* ptau, size_t len, const char* name, const uint8_t* secrets, void** out, size_t* out_len, void* hash64,
                        gw_status_t* status) {
    if (!out || !out_len || !hash64 || (!ptau && len)) return fail2(status, "gwb_ptau_contribute: NULL argument");
    *out = nullptr;
    *out_len = 0;
    try {
        return contribute((const uint8_t*)ptau, len, name, secrets, out, out_len, (uint8_t*)hash64, status);
    } catch (const std::bad_alloc&) {
        return fail2(status, "ptau contribute: out of host memory");
    }
}

int gwb_ptau_beacon(const void* ptau, size_t len, const char* name, const void* beacon_hash, size_t hash_len, uint32_t iterations_exp, void** out,
                    size_t* out_len, void* hash64, gw_status_t* status) {
    if (!out || !out_len || !hash64 || (!ptau && len) || (!beacon_hash && hash_len)) return fail2(status, "gwb_ptau_beacon: NULL argument");
    *out = nullptr;
    *out_len = 0;
    try {
        return beacon((const uint8_t*)ptau, len, name, (const uint8_t*)beacon_hash, hash_len, iterations_exp, out, out_len, (uint8_t*)hash64, status);
    } catch (const std::bad_alloc&) {
        return fail2(status, "beacon: out of host memory");
    }
}

int gwb_ptau_contribute_phase_ms(float* ms) { return g_phases.read(ms); }

}  // extern "C"
