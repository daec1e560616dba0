// Groth16 circuit-specific setup on gfx950 (include/graph_witness_groth16_setup.h has the definition): from the `.r1cs` handle
// and a trapdoor (tau, alpha, beta, gamma, delta), the proving key as a `.zkey` image.  Every field value on the device is in
// Montgomery form until the key scalars are written (canonical, the form the fixed-base kernel takes).
//
// Lagrange values.  L_k and M_j for k, j < n are one array of 2n values x -> z x / (tau - x) (x = w^k, then g w^j).  A thread
// takes INV_CHUNK consecutive values: the denominators, their running products, one Fermat inversion, and the walk back
// (Montgomery's trick), so an inversion is shared by INV_CHUNK values.  tau^2n != 1 (checked on the host): no denominator is 0.
//
// Column sums.  The handle stores the matrices by constraint; the host builds the by-wire transpose once per call: the terms
// of every (wire, matrix) column, cut into segments of at most `segment` terms.  One thread sums a segment (a term is a
// gather of L_k and, for a general coefficient, one product), then one thread per wire adds its segments' partial sums
// (additions only) and, for i <= nPub, L_{nC+i}.  Field addition is exact, so duplicate terms simply add.  The constant wire
// of a real circuit occurs in most constraints: its column is thousands of segments, summed by as many threads.
// Splitting decision, on the measured time: on the authV2-class system (333 233 terms, n = 2^17) the column sums take 0.56 ms
// with segments of 64 terms and 40.9 ms with unsplit columns (CWC_GROTH16_SETUP_SEGMENT=0; tools/gpu_groth16_setup.py,
// profiles/groth16_setup.txt): unsplit, the longest column runs on one lane and sets the time of the phase.  Columns are
// split, 64 terms per segment.
//
// Key scalars.  gamma^-1 and delta^-1 are computed once on the host (two inversions per call); one kernel writes the G1
// scalar list [A: nW][B1: nW][C: nW - nPub - 1][H: n][IC: nPub + 1][alpha, beta, delta] and the G2 list [B2: nW][beta, gamma,
// delta].
//
// Fixed-base multiplication.  Per generator a table T[w][d] = d 2^(8 w) G (affine, 32 windows of 256 entries: 512 KiB for
// G1, 1 MiB for G2), built once per process and device.  One thread per scalar adds the table entries of its nonzero bytes
// with mixed additions (xyzz_add_affine, which doubles or cancels where the operands require it); a zero byte is skipped.
//
// To affine.  x = X / ZZ and y = Y / ZZZ need 1 / (ZZ ZZZ) only (1 / ZZ = ZZZ / (ZZ ZZZ)); a thread shares one inversion among
// INV_CHUNK consecutive points by Montgomery's trick.  A point at infinity enters the running product as 1 and is written as
// zero bytes, so it cannot poison the others.  The running products wait in the output slots, which the walk back overwrites.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage for gfx950; every kernel: 0 bytes of scratch, no VGPR spill):
//   gen_mul_kernel<G1> 107 VGPRs, 4 waves / SIMD      gen_mul_kernel<G2> 220 VGPRs, 2 waves / SIMD
//   affine_kernel<G1>   90 VGPRs, 5 waves / SIMD      affine_kernel<G2>  256 VGPRs + 19 AGPRs, 1 wave / SIMD
//   table_fill_kernel<G2> 256 VGPRs + 33 AGPRs (once per process); the Fr kernels 59 to 86 VGPRs.
// A G2 accumulator in XYZZ is 64 VGPRs before temporaries.  Launch bounds of 256 threads are one wave per SIMD, which leaves
// the allocator all 512 registers, so nothing spills; a smaller block would not raise the G2 kernels' occupancy, which the
// register count sets.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/graph_witness_groth16_setup.h"
#include "bn254_points_gfx950.hpp"
#include "groth16_internal.hpp"
#include "lincomb.hpp"
#include "setup_internal.hpp"

using namespace cwc_r1cs;
using namespace cwc_g16;
using cwc::Fr;
using cwc_setup::Columns;
using cwc_setup::KeyLayout;

namespace {

constexpr uint32_t THREADS = 256;
constexpr uint32_t INV_CHUNK = 16;    // values per shared inversion
constexpr uint32_t N_WIN = 32;        // 8-bit windows of a 256-bit scalar
constexpr uint32_t TABLE_POINTS = N_WIN * 256;
constexpr uint32_t SEGMENT_DEFAULT = 64;

// lag[e] = z x / (tau - x): e < n: x = w^e, z = zf (L_e); e >= n: x = g w^(e - n), z = zf2 (M_{e-n}).  pref is a work array.
__global__ __launch_bounds__(THREADS) void setup_lagrange_kernel(Fr* __restrict__ lag, Fr* __restrict__ pref, uint32_t log_n, Pows wp, Fr g,
                                                                 Fr tau, Fr zf, Fr zf2) {
    const uint32_t n = 1u << log_n, total = 2u * n;
    const uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * INV_CHUNK;
    if (first >= total) return;
    const uint32_t e0 = (uint32_t)first, e1 = total - e0 < INV_CHUNK ? total : e0 + INV_CHUNK;
    Fr x = e0 >= n ? g : cwc::fr_one();
    for (uint32_t b = 0; b < log_n; ++b)
        if ((e0 >> b) & 1u) x = cwc::fr_mul(x, wp.v[b]);
    Fr acc = cwc::fr_one();
    for (uint32_t e = e0; e < e1; ++e) {
        if (e == n) x = g;  // a chunk that holds the end of L and the start of M (n < INV_CHUNK)
        const Fr d = cwc::fr_sub(tau, x);
        lag[e] = d;
        pref[e] = acc;
        acc = cwc::fr_mul(acc, d);
        x = cwc::fr_mul(x, wp.v[0]);
    }
    Fr inv = cwc::fr_inv_fermat(acc);
    for (uint32_t e = e1; e-- > e0;) {
        const Fr d = lag[e];
        const Fr ie = cwc::fr_mul(inv, pref[e]);
        inv = cwc::fr_mul(inv, d);
        lag[e] = cwc::fr_mul(cwc::fr_mul(e < n ? zf : zf2, cwc::fr_sub(tau, d)), ie);
    }
}

// part[s] = sum of the terms ent[seg_off[s] .. seg_off[s + 1]) of one (wire, matrix) column: coefficient x L_k
__global__ __launch_bounds__(THREADS) void setup_segments_kernel(const uint32_t* __restrict__ ent, const uint32_t* __restrict__ cidx,
                                                                 const Fr* __restrict__ coef, const Fr* __restrict__ lag,
                                                                 const uint32_t* __restrict__ seg_off, uint32_t n_seg, Fr* __restrict__ part) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    Fr acc = cwc::fr_zero();
    for (uint32_t j = seg_off[s], end = seg_off[s + 1]; j < end; ++j) {
        const uint32_t e = ent[j], kind = e >> 30;
        const Fr l = lag[e & WIRE_MASK];
        if (kind == KIND_GENERAL)
            acc = cwc::fr_add(acc, cwc::fr_mul(l, coef[cidx[j]]));
        else
            acc = kind == KIND_PLUS ? cwc::fr_add(acc, l) : cwc::fr_sub(acc, l);
    }
    part[s] = acc;
}

// uvw[m nW + i] = the sum of wire i's segments of matrix m (seg_key = 3 wire + m), plus L_{nC+i} in u for i <= nPub
__global__ __launch_bounds__(THREADS) void setup_wires_kernel(const Fr* __restrict__ part, const uint32_t* __restrict__ seg_key,
                                                              const uint32_t* __restrict__ wire_seg, const Fr* __restrict__ lag, uint32_t n_wires,
                                                              uint32_t n_constraints, uint32_t n_pub, Fr* __restrict__ uvw) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_wires) return;
    Fr u = cwc::fr_zero(), v = u, w = u;
    for (uint32_t s = wire_seg[i], end = wire_seg[i + 1]; s < end; ++s) {
        const Fr p = part[s];
        const uint32_t m = seg_key[s] - 3u * i;
        if (m == 0)
            u = cwc::fr_add(u, p);
        else if (m == 1)
            v = cwc::fr_add(v, p);
        else
            w = cwc::fr_add(w, p);
    }
    if (i <= n_pub) u = cwc::fr_add(u, lag[n_constraints + i]);
    uvw[i] = u;
    uvw[(size_t)n_wires + i] = v;
    uvw[2 * (size_t)n_wires + i] = w;
}

struct KeyConsts {
    Fr alpha_m, beta_m, gamma_inv_m, delta_inv_m;  // Montgomery form
};

// the canonical scalar lists: s1 = [A][B1][C][H][IC][alpha, beta, delta], s2 = [B2][beta, gamma, delta] (the host copies the
// three trapdoor values at the end of each)
__global__ __launch_bounds__(THREADS) void setup_scalars_kernel(const Fr* __restrict__ uvw, const Fr* __restrict__ lag, uint32_t n_wires,
                                                                uint32_t n_pub, uint32_t n, KeyConsts k, Fr* __restrict__ s1, Fr* __restrict__ s2) {
    const KeyLayout at{n_wires, n_pub, n};
    const uint32_t total = n_wires > n ? n_wires : n;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        if (i < n_wires) {
            const Fr u = uvw[i], v = uvw[(size_t)n_wires + i], w = uvw[2 * (size_t)n_wires + i];
            const Fr vc = cwc::fr_from_mont(v);
            s1[i] = cwc::fr_from_mont(u);
            s1[at.b1() + i] = vc;
            s2[i] = vc;
            const Fr t = cwc::fr_add(cwc::fr_add(cwc::fr_mul(k.beta_m, u), cwc::fr_mul(k.alpha_m, v)), w);
            if (i <= n_pub)
                s1[at.ic() + i] = cwc::fr_from_mont(cwc::fr_mul(t, k.gamma_inv_m));
            else
                s1[at.c() + (i - n_pub - 1)] = cwc::fr_from_mont(cwc::fr_mul(t, k.delta_inv_m));
        }
        if (i < n) s1[at.h() + i] = cwc::fr_from_mont(cwc::fr_mul(lag[(size_t)n + i], k.delta_inv_m));
    }
}

// ---- the tables of generator multiples ------------------------------------------------------------------------------------

// bases[w] = 2^(8 w) G
template <class T>
__global__ __launch_bounds__(64) void table_bases_kernel(Affine<T> gen, Affine<T>* __restrict__ bases) {
    const uint32_t w = threadIdx.x;
    if (w >= N_WIN) return;
    Xyzz<T> p{gen.x, gen.y, T::one(), T::one()};
    for (uint32_t d = 0; d < 8 * w; ++d) p = xyzz_dbl(p);
    bases[w] = xyzz_to_affine(p);
}

// table[256 w + d] = d bases[w] (d = 0: unused, zero bytes)
template <class T>
__global__ __launch_bounds__(THREADS) void table_fill_kernel(const Affine<T>* __restrict__ bases, Affine<T>* __restrict__ table) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= TABLE_POINTS) return;
    const uint32_t d = id & 255u;
    const Affine<T> b = bases[id >> 8];
    Xyzz<T> acc = xyzz_inf<T>();
    for (int bit = 7; bit >= 0; --bit) {
        acc = xyzz_dbl(acc);
        if ((d >> bit) & 1u) acc = xyzz_add_affine(acc, b);
    }
    table[id] = xyzz_to_affine(acc);
}

// out[t] = k_t G for canonical k_t (values >= r reduced): the table entries of the nonzero bytes of k_t
template <class T>
__global__ __launch_bounds__(THREADS) void gen_mul_kernel(const Fr* __restrict__ scalars, uint32_t n, const Affine<T>* __restrict__ table,
                                                          Xyzz<T>* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    Fr k = reduce_any(scalars[t]);
    Xyzz<T> acc = xyzz_inf<T>();
    for (uint32_t w = 0; w < N_WIN; w += 4) {
        uint32_t word = k.v[0];  // words move down into k.v[0] (constant indices: k stays in registers)
        for (uint32_t b = 0; b < 4; ++b) {
            const uint32_t d = word & 255u;
            word >>= 8;
            if (d) acc = xyzz_add_affine(acc, table[((w + b) << 8) + d]);
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) k.v[i] = k.v[i + 1];
    }
    out[t] = acc;
}

// pts -> affine coordinates (x, y; Montgomery bytes as the zkey stores them, or canonical), infinity = zero bytes
template <class T>
__global__ __launch_bounds__(THREADS) void affine_kernel(const Xyzz<T>* __restrict__ pts, uint32_t n, uint8_t* __restrict__ out, uint32_t canonical) {
    using E = typename T::E;
    constexpr size_t PB = 2 * sizeof(E);  // bytes per output point
    const uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * INV_CHUNK;
    if (first >= n) return;
    const uint32_t e0 = (uint32_t)first, e1 = n - e0 < INV_CHUNK ? n : e0 + INV_CHUNK;
    E acc = T::one();
    for (uint32_t e = e0; e < e1; ++e) {
        *reinterpret_cast<E*>(out + e * PB) = acc;  // the product of the points before e, until the walk back
        const E zz = pts[e].ZZ, zzz = pts[e].ZZZ;
        if (!T::is_zero(zz)) acc = T::mul(acc, T::mul(zz, zzz));
    }
    E inv = T::inv(acc);
    for (uint32_t e = e1; e-- > e0;) {
        const Xyzz<T> p = pts[e];
        uint8_t* o = out + e * PB;
        if (xyzz_is_inf(p)) {
            put_coords<T>(o, T::zero(), T::zero(), false);
            continue;
        }
        const E ie = T::mul(inv, *reinterpret_cast<const E*>(o));  // 1 / (ZZ ZZZ)
        inv = T::mul(inv, T::mul(p.ZZ, p.ZZZ));
        put_coords<T>(o, T::mul(p.X, T::mul(p.ZZZ, ie)), T::mul(p.Y, T::mul(p.ZZ, ie)), canonical != 0);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------

// The tables of one device: built at the first use in the process and kept until it ends.
struct Tables {
    void *g1 = nullptr, *g2 = nullptr;
};
constexpr int MAX_DEVICES = 64;
std::mutex g_tables_mutex;
Tables g_tables[MAX_DEVICES];

template <class T>
hipError_t build_table(const Affine<T>& gen, void** out, hipStream_t s) {
    DeviceBuf bases, table;
    hipError_t e = bases.alloc(N_WIN * sizeof(Affine<T>));
    if (e == hipSuccess) e = table.alloc(TABLE_POINTS * sizeof(Affine<T>));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(table_bases_kernel<T>, dim3(1), dim3(64), 0, s, gen, bases.as<Affine<T>>());
        hipLaunchKernelGGL(table_fill_kernel<T>, dim3(blocks_for(TABLE_POINTS, THREADS)), dim3(THREADS), 0, s, bases.as<const Affine<T>>(),
                           table.as<Affine<T>>());
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) return e;
    *out = table.release();  // kept until the process ends, by design: the table leaves its owner here
    return hipSuccess;
}

bool ensure_tables(Tables& t, std::string& err) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0 || dev >= MAX_DEVICES) {
        err = e != hipSuccess ? hip_err("finding the current device", e) : "groth16 setup: device index " + std::to_string(dev) + " is not supported";
        return false;
    }
    std::lock_guard<std::mutex> lock(g_tables_mutex);
    Tables& g = g_tables[dev];
    if (!g.g2) {
        Stream s;
        e = s.create();
        if (e == hipSuccess && !g.g1) e = build_table<G1>(g1_generator(), &g.g1, s);
        if (e == hipSuccess) e = build_table<G2>(g2_generator(), &g.g2, s);
        if (e != hipSuccess) {
            err = hip_err("building the tables of generator multiples", e);
            return false;
        }
    }
    t = g;
    return true;
}

template <class T>
void enqueue_affine(const void* d_xyzz, uint32_t n, uint8_t* d_out, bool canonical, hipStream_t s) {
    hipLaunchKernelGGL(affine_kernel<T>, dim3(blocks_for(((uint64_t)n + INV_CHUNK - 1) / INV_CHUNK, THREADS)), dim3(THREADS), 0, s, (const Xyzz<T>*)d_xyzz, n,
                       d_out, canonical ? 1u : 0u);
}

}  // namespace

namespace cwc_setup {

uint32_t segment_terms() {  // CWC_GROTH16_SETUP_SEGMENT: terms per segment of a column; 0 = columns are not split (measurement aid)
    const char* s = getenv("CWC_GROTH16_SETUP_SEGMENT");
    if (!s || !*s) return SEGMENT_DEFAULT;
    const unsigned long long v = strtoull(s, nullptr, 10);
    return v == 0 || v > 0xffffffffull ? 0xffffffffu : (uint32_t)v;
}

// The by-wire transpose of the handle's matrices (Columns: setup_internal.hpp)
void transpose(const gwb_r1cs* r, uint32_t segment, Columns& c) {
    const uint32_t nw = r->info.n_wires, nc = r->info.n_constraints;
    const size_t n_terms = r->sys.fac.size();
    std::vector<uint32_t> start(3 * (size_t)nw + 1, 0);
    for (uint32_t k = 0; k < nc; ++k)
        for (uint32_t m = 0; m < 3; ++m)
            for (uint32_t j = r->sys.rowptr[3 * (size_t)k + m]; j < r->sys.rowptr[3 * (size_t)k + m + 1]; ++j)
                ++start[3 * (size_t)(r->sys.fac[j] & WIRE_MASK) + m + 1];
    for (size_t i = 1; i < start.size(); ++i) start[i] += start[i - 1];
    c.ent.resize(n_terms);
    c.cidx.resize(n_terms);
    std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    for (uint32_t k = 0; k < nc; ++k)
        for (uint32_t m = 0; m < 3; ++m)
            for (uint32_t j = r->sys.rowptr[3 * (size_t)k + m]; j < r->sys.rowptr[3 * (size_t)k + m + 1]; ++j) {
                const uint32_t f = r->sys.fac[j], at = fill[3 * (size_t)(f & WIRE_MASK) + m]++;
                c.ent[at] = r->sys.perm[k] | (f & ~WIRE_MASK);
                c.cidx[at] = r->sys.cidx[j];
            }
    c.wire_seg.assign((size_t)nw + 1, 0);
    for (uint32_t i = 0; i < nw; ++i) {
        c.wire_seg[i] = (uint32_t)c.seg_key.size();
        for (uint32_t m = 0; m < 3; ++m) {
            const uint32_t key = 3 * i + m;
            for (uint32_t at = start[key]; at < start[key + 1];) {
                c.seg_off.push_back(at);
                c.seg_key.push_back(key);
                at = start[key + 1] - at > segment ? at + segment : start[key + 1];
            }
        }
    }
    c.wire_seg[nw] = (uint32_t)c.seg_key.size();
    c.seg_off.push_back((uint32_t)n_terms);
}

size_t columns_bytes(const Columns& c, size_t n_coef) {
    Carve cw;
    for (size_t bytes : {c.ent.size() * 4, c.cidx.size() * 4, n_coef * 32, c.seg_off.size() * 4, c.seg_key.size() * 4, c.wire_seg.size() * 4}) cw.take(bytes);
    return cw.o;
}

// the arrays in columns_bytes' order
DeviceColumns upload_columns(const Columns& c, const std::vector<Fr>& coef, uint8_t* at, hipStream_t s, hipError_t& e) {
    Carve cw;
    auto up = [&](const void* src, size_t bytes) {
        uint8_t* dst = at + cw.take(bytes);
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
        return dst;
    };
    DeviceColumns d;
    d.ent = (const uint32_t*)up(c.ent.data(), c.ent.size() * 4);
    d.cidx = (const uint32_t*)up(c.cidx.data(), c.cidx.size() * 4);
    d.coef = (const Fr*)up(coef.data(), coef.size() * 32);
    d.seg_off = (const uint32_t*)up(c.seg_off.data(), c.seg_off.size() * 4);
    d.seg_key = (const uint32_t*)up(c.seg_key.data(), c.seg_key.size() * 4);
    d.wire_seg = (const uint32_t*)up(c.wire_seg.data(), c.wire_seg.size() * 4);
    d.n_seg = (uint32_t)c.seg_key.size();
    return d;
}

void enqueue_affine_g1(const void* d_xyzz, uint32_t n, uint8_t* d_out, bool canonical, void* stream) {
    enqueue_affine<G1>(d_xyzz, n, d_out, canonical, (hipStream_t)stream);
}
void enqueue_affine_g2(const void* d_xyzz, uint32_t n, uint8_t* d_out, bool canonical, void* stream) {
    enqueue_affine<G2>(d_xyzz, n, d_out, canonical, (hipStream_t)stream);
}

}  // namespace cwc_setup

using namespace cwc_setup;

namespace {

// Host copies of the trapdoor and what is derived from it; zeroed when the call leaves.
struct Secrets {
    Fr tau, alpha, beta, gamma, delta;  // canonical
    Fr tau_m, zf, zf2;
    KeyConsts k;
    ~Secrets() { explicit_bzero(this, sizeof *this); }
};

Fr fr_pow2k(Fr x, uint32_t k) {  // x^(2^k)
    for (uint32_t i = 0; i < k; ++i) x = cwc::fr_mul(x, x);
    return x;
}

// tau^2n = 1: tau is a point of the n domain or of its odd coset, where a Lagrange denominator vanishes
bool tau_on_domain(const Fr& tau, uint32_t p) { return cwc::u256_eq(fr_pow2k(cwc::fr_to_mont(tau), p + 1), cwc::fr_one()); }

bool take_trapdoor(const gwb_groth16_trapdoor_t* t, uint32_t p, Secrets& s, std::string& err) {
    Fr* dst[5] = {&s.tau, &s.alpha, &s.beta, &s.gamma, &s.delta};
    static const char* names[5] = {"tau", "alpha", "beta", "gamma", "delta"};
    if (t) {
        const uint8_t* src[5] = {t->tau, t->alpha, t->beta, t->gamma, t->delta};
        for (int i = 0; i < 5; ++i) {
            memcpy(dst[i]->v, src[i], 32);
            if (cwc::u256_is_zero(*dst[i])) {
                err = std::string("groth16 setup: trapdoor value ") + names[i] + " is 0 (each value must lie in [1, r))";
                return false;
            }
            if (!cwc::u256_lt(*dst[i], cwc::fr_p())) {
                err = std::string("groth16 setup: trapdoor value ") + names[i] + " is not below r (each value must lie in [1, r))";
                return false;
            }
        }
        if (tau_on_domain(s.tau, p)) {
            err = "groth16 setup: trapdoor value tau satisfies tau^(2n) = 1 for the domain n = 2^" + std::to_string(p) +
                  ": it is a point of the QAP domain or of its coset, where a Lagrange denominator is 0";
            return false;
        }
        return true;
    }
    for (int i = 0; i < 5; ++i) {
        do {
            if (!draw_fr(*dst[i], err)) return false;
        } while (cwc::u256_is_zero(*dst[i]) || (i == 0 && tau_on_domain(*dst[i], p)));
    }
    return true;
}

// 1 / 2^k = r - (r - 1) / 2^k for 2^k dividing r - 1; Montgomery form
Fr inv_pow2(uint32_t k) {
    Fr rm1 = cwc::fr_p(), out;
    rm1.v[0] -= 1;  // r is odd
    cwc::u256_sub(out, cwc::fr_p(), cwc::u256_shr(rm1, k));
    return cwc::fr_to_mont(out);
}

void derive(Secrets& s, uint32_t p) {
    s.tau_m = cwc::fr_to_mont(s.tau);
    const Fr tn = fr_pow2k(s.tau_m, p), t2n = cwc::fr_mul(tn, tn);
    s.zf = cwc::fr_mul(cwc::fr_sub(tn, cwc::fr_one()), inv_pow2(p));
    s.zf2 = cwc::fr_mul(cwc::fr_sub(t2n, cwc::fr_one()), inv_pow2(p + 1));
    s.k.alpha_m = cwc::fr_to_mont(s.alpha);
    s.k.beta_m = cwc::fr_to_mont(s.beta);
    s.k.gamma_inv_m = cwc::fr_inv_fermat(cwc::fr_to_mont(s.gamma));  // the call's two field inversions
    s.k.delta_inv_m = cwc::fr_inv_fermat(cwc::fr_to_mont(s.delta));
}

PhaseTimes<5> g_phases;

void put32(std::vector<uint8_t>& v, uint32_t x) { v.insert(v.end(), (const uint8_t*)&x, (const uint8_t*)&x + 4); }
void put64(std::vector<uint8_t>& v, uint64_t x) { v.insert(v.end(), (const uint8_t*)&x, (const uint8_t*)&x + 8); }
void put_fr(std::vector<uint8_t>& v, const Fr& x) { v.insert(v.end(), (const uint8_t*)x.v, (const uint8_t*)x.v + 32); }

}  // namespace

// section 4 as snarkjs `zkey new` lays it out (values value R^2 mod r)
bool cwc_setup::coefficients_section(const gwb_r1cs* r, std::vector<uint8_t>& out, std::string& err) {
    const uint32_t nc = r->info.n_constraints, n_pub = r->info.n_pub_out + r->info.n_pub_in;
    const uint64_t count = r->info.n_factors_a + r->info.n_factors_b + n_pub + 1;
    if (count > 0xffffffffull) {
        err = "groth16 setup: more than 2^32 - 1 coefficients in section 4";
        return false;
    }
    const Fr one_rr = cwc::fr_r2(), minus_rr = cwc::fr_neg(one_rr);
    std::vector<Fr> coef_rr(r->sys.coef.size());
    for (size_t i = 0; i < coef_rr.size(); ++i) coef_rr[i] = cwc::fr_to_mont(r->sys.coef[i]);  // c R -> c R^2
    std::vector<uint32_t> pos(nc);  // file index -> position in the handle's order
    for (uint32_t k = 0; k < nc; ++k) pos[r->sys.perm[k]] = k;
    out.reserve(4 + count * 44);
    put32(out, (uint32_t)count);
    for (uint32_t k = 0; k < nc; ++k)
        for (uint32_t m = 0; m < 2; ++m)
            for (uint32_t j = r->sys.rowptr[3 * (size_t)pos[k] + m]; j < r->sys.rowptr[3 * (size_t)pos[k] + m + 1]; ++j) {
                const uint32_t f = r->sys.fac[j], kind = f >> 30;
                put32(out, m);
                put32(out, k);
                put32(out, f & WIRE_MASK);
                put_fr(out, kind == KIND_PLUS ? one_rr : kind == KIND_MINUS ? minus_rr : coef_rr[r->sys.cidx[j]]);
            }
    for (uint32_t s = 0; s <= n_pub; ++s) {
        put32(out, 0);
        put32(out, nc + s);
        put32(out, s);
        put_fr(out, one_rr);
    }
    return true;
}

namespace {

void put_section(std::vector<uint8_t>& v, uint32_t id, const uint8_t* p, size_t n) {
    put32(v, id);
    put64(v, n);
    v.insert(v.end(), p, p + n);
}

}  // namespace

// -- the file: sections 1 to 10 in ascending order
int cwc_setup::write_zkey(const KeyPoints& k, const std::vector<uint8_t>& sec4, void** zkey, size_t* zkey_len, gw_status_t* status) {
    const uint32_t nw = k.n_wires, n_pub = k.n_pub, n = k.n;
    std::vector<uint8_t> hdr;
    put32(hdr, 32);
    put_fr(hdr, fq_p());
    put32(hdr, 32);
    put_fr(hdr, cwc::fr_p());
    put32(hdr, nw);
    put32(hdr, n_pub);
    put32(hdr, n);
    hdr.insert(hdr.end(), k.alpha1, k.alpha1 + G1_BYTES);
    hdr.insert(hdr.end(), k.beta1, k.beta1 + G1_BYTES);
    hdr.insert(hdr.end(), k.beta2, k.beta2 + G2_BYTES);
    hdr.insert(hdr.end(), k.gamma2, k.gamma2 + G2_BYTES);
    hdr.insert(hdr.end(), k.delta1, k.delta1 + G1_BYTES);
    hdr.insert(hdr.end(), k.delta2, k.delta2 + G2_BYTES);
    const size_t n1 = 3 * (size_t)nw + n, points = n1 * G1_BYTES + (size_t)nw * G2_BYTES;
    std::vector<uint8_t> out;
    out.reserve(12 + 10 * 12 + 4 + hdr.size() + sec4.size() + points + 68);
    out.insert(out.end(), {'z', 'k', 'e', 'y'});
    put32(out, 1);
    put32(out, 10);
    const uint32_t protocol = 1;
    put_section(out, 1, (const uint8_t*)&protocol, 4);
    put_section(out, 2, hdr.data(), hdr.size());
    put_section(out, 3, k.ic, (size_t)(n_pub + 1) * G1_BYTES);
    put_section(out, 4, sec4.data(), sec4.size());
    put_section(out, 5, k.a, (size_t)nw * G1_BYTES);
    put_section(out, 6, k.b1, (size_t)nw * G1_BYTES);
    put_section(out, 7, k.b2, (size_t)nw * G2_BYTES);
    put_section(out, 8, k.c, (size_t)(nw - n_pub - 1) * G1_BYTES);
    put_section(out, 9, k.h, (size_t)n * G1_BYTES);
    const uint8_t no_contributions[68] = {};  // 64 zero bytes in place of the circuit hash, then u32 0 contributions
    put_section(out, 10, no_contributions, sizeof no_contributions);
    void* buf = malloc(out.size());
    if (!buf) return fail(status, "groth16 setup: out of host memory");
    memcpy(buf, out.data(), out.size());
    *zkey = buf;
    *zkey_len = out.size();
    set_ok(status);
    return 0;
}

namespace {

int setup(gwb_r1cs* r, const gwb_groth16_trapdoor_t* trapdoor, void** zkey, size_t* zkey_len, gw_status_t* status) {
    gwb_r1cs_qap_info_t qi;
    if (gwb_r1cs_qap_info(r, &qi, status) != 0) return 1;
    const uint32_t p = qi.domain_power, n = (uint32_t)qi.domain_size;
    const uint32_t nw = r->info.n_wires, nc = r->info.n_constraints, n_pub = r->info.n_pub_out + r->info.n_pub_in;
    std::string err;
    Secrets sec;
    if (!take_trapdoor(trapdoor, p, sec, err)) return fail(status, err);
    derive(sec, p);
    const KeyLayout at{nw, n_pub, n};
    const uint64_t n1 = at.n1() + 3, n2 = (uint64_t)nw + 3;  // the header's scalars at the end of both lists
    if (n1 > 0x7fffffffull) return fail(status, "groth16 setup: more than 2^31 - 1 points");
    std::vector<uint8_t> sec4;
    if (!coefficients_section(r, sec4, err)) return fail(status, err);
    Columns col;
    transpose(r, segment_terms(), col);
    const uint32_t n_seg = (uint32_t)col.seg_key.size();

    Tables tab;
    if (!ensure_tables(tab, err)) return fail(status, err);
    SetupDevice<6> D;
    Carve cs, cw;
    const size_t o_lag = cs.take(2ull * n * 32), o_pref = cs.take(2ull * n * 32), o_part = cs.take((size_t)n_seg * 32),
                 o_uvw = cs.take(3ull * nw * 32), o_s1 = cs.take(n1 * 32), o_s2 = cs.take(n2 * 32);
    const size_t o_col = cw.take(columns_bytes(col, r->sys.coef.size())), o_x1 = cw.take(n1 * sizeof(Xyzz<G1>)),
                 o_x2 = cw.take(n2 * sizeof(Xyzz<G2>)), o_p1 = cw.take(n1 * G1_BYTES), o_p2 = cw.take(n2 * G2_BYTES);
    hipError_t e = D.open(cs.o, std::max<size_t>(cw.o, 256));
    if (e != hipSuccess) return fail(status, hip_err("allocating the setup workspace", e));
    uint8_t *S = D.secret.as<uint8_t>(), *W = D.work.as<uint8_t>();
    const DeviceColumns dc = upload_columns(col, r->sys.coef, W + o_col, D.s, e);
    // the header's scalars, at the end of the two scalar lists
    Fr *lag = (Fr*)(S + o_lag), *s1 = (Fr*)(S + o_s1), *s2 = (Fr*)(S + o_s2);
    Fr k1s[3] = {sec.alpha, sec.beta, sec.delta}, k2s[3] = {sec.beta, sec.gamma, sec.delta};
    if (e == hipSuccess) e = hipMemcpyAsync(s1 + (n1 - 3), k1s, sizeof k1s, hipMemcpyHostToDevice, D.s);
    if (e == hipSuccess) e = hipMemcpyAsync(s2 + nw, k2s, sizeof k2s, hipMemcpyHostToDevice, D.s);
    if (e == hipSuccess) e = hipStreamSynchronize(D.s);  // the copies have left the host arrays
    explicit_bzero(k1s, sizeof k1s);
    explicit_bzero(k2s, sizeof k2s);
    if (e != hipSuccess) return fail(status, hip_err("uploading the transposed constraint matrices", e));

    Fr wn, g;
    qap_roots(p, wn, g);
    D.ev.record(0, D.s);
    hipLaunchKernelGGL(setup_lagrange_kernel, dim3(blocks_for((2ull * n + INV_CHUNK - 1) / INV_CHUNK, THREADS)), dim3(THREADS), 0, D.s, lag,
                       (Fr*)(S + o_pref), p, powers_of(wn), g, sec.tau_m, sec.zf, sec.zf2);
    D.ev.record(1, D.s);
    if (n_seg)
        hipLaunchKernelGGL(setup_segments_kernel, dim3(blocks_for(n_seg, THREADS)), dim3(THREADS), 0, D.s, dc.ent, dc.cidx, dc.coef, (const Fr*)lag, dc.seg_off,
                           n_seg, (Fr*)(S + o_part));
    hipLaunchKernelGGL(setup_wires_kernel, dim3(blocks_for(nw, THREADS)), dim3(THREADS), 0, D.s, (const Fr*)(S + o_part), dc.seg_key, dc.wire_seg,
                       (const Fr*)lag, nw, nc, n_pub, (Fr*)(S + o_uvw));
    D.ev.record(2, D.s);
    hipLaunchKernelGGL(setup_scalars_kernel, dim3(std::min<uint32_t>(blocks_for(std::max(nw, n), THREADS), 4096)), dim3(THREADS), 0, D.s,
                       (const Fr*)(S + o_uvw), (const Fr*)lag, nw, n_pub, n, sec.k, s1, s2);
    D.ev.record(3, D.s);
    hipLaunchKernelGGL(gen_mul_kernel<G1>, dim3(blocks_for(n1, THREADS)), dim3(THREADS), 0, D.s, (const Fr*)s1, (uint32_t)n1, (const Affine<G1>*)tab.g1,
                       (Xyzz<G1>*)(W + o_x1));
    D.ev.record(4, D.s);
    hipLaunchKernelGGL(gen_mul_kernel<G2>, dim3(blocks_for(n2, THREADS)), dim3(THREADS), 0, D.s, (const Fr*)s2, (uint32_t)n2, (const Affine<G2>*)tab.g2,
                       (Xyzz<G2>*)(W + o_x2));
    enqueue_affine<G1>(W + o_x1, (uint32_t)n1, W + o_p1, false, D.s);
    enqueue_affine<G2>(W + o_x2, (uint32_t)n2, W + o_p2, false, D.s);
    D.ev.record(5, D.s);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(status, hip_err("launching the setup kernels", e));
    std::vector<uint8_t> p1(n1 * G1_BYTES), p2(n2 * G2_BYTES);
    e = hipMemcpyAsync(p1.data(), W + o_p1, p1.size(), hipMemcpyDeviceToHost, D.s);
    if (e == hipSuccess) e = hipMemcpyAsync(p2.data(), W + o_p2, p2.size(), hipMemcpyDeviceToHost, D.s);
    if (e == hipSuccess) e = hipMemsetAsync(D.secret.as(), 0, D.secret_bytes, D.s);
    if (e == hipSuccess) e = hipStreamSynchronize(D.s);
    if (e != hipSuccess) return fail(status, hip_err("running the setup", e));
    g_phases.record(D.ev);

    const uint8_t *a = p1.data(), *b1 = a + at.b1() * G1_BYTES, *c = a + at.c() * G1_BYTES, *h = a + at.h() * G1_BYTES,
                  *ic = a + at.ic() * G1_BYTES, *k1 = a + at.n1() * G1_BYTES;
    const uint8_t *b2 = p2.data(), *k2 = b2 + (size_t)nw * G2_BYTES;
    const KeyPoints kp{nw, n_pub, n, k1, k1 + G1_BYTES, k2, k2 + G2_BYTES, k1 + 2 * G1_BYTES, k2 + 2 * G2_BYTES, ic, a, b1, b2, c, h};
    return write_zkey(kp, sec4, zkey, zkey_len, status);
}

}  // namespace

extern "C" {

int gwb_groth16_setup(gwb_r1cs_t* r, const gwb_groth16_trapdoor_t* trapdoor, void** zkey, size_t* zkey_len, gw_status_t* status) {
    if (!r || !zkey || !zkey_len) return fail(status, "gwb_groth16_setup: NULL argument");
    *zkey = nullptr;
    *zkey_len = 0;
    try {
        return setup(r, trapdoor, zkey, zkey_len, status);
    } catch (const std::bad_alloc&) {
        return fail(status, "groth16 setup: out of host memory");
    }
}

void gwb_groth16_setup_free(void* zkey) { free(zkey); }

int gwb_bn254_gen_mul_batch_device(const void* d_scalars, size_t n, uint32_t group, void* d_points, void* hip_stream, gw_status_t* status) {
    if (n && (!d_scalars || !d_points)) return fail(status, "gwb_bn254_gen_mul_batch_device: NULL argument");
    if (group != 1 && group != 2) return fail(status, "gwb_bn254_gen_mul_batch_device: group " + std::to_string(group) + " (1 or 2 expected)");
    if (n > 0x7fffffffull) return fail(status, "gwb_bn254_gen_mul_batch_device: n above 2^31 - 1");
    if (n == 0) {
        set_ok(status);
        return 0;
    }
    std::string err;
    Tables tab;
    if (!ensure_tables(tab, err)) return fail(status, err);
    hipStream_t s = (hipStream_t)hip_stream;
    void* ws = nullptr;
    hipError_t e = hipMallocAsync(&ws, n * (group == 1 ? sizeof(Xyzz<G1>) : sizeof(Xyzz<G2>)), s);
    if (e != hipSuccess) return fail(status, hip_err("allocating the multiplication workspace", e));
    if (group == 1) {
        hipLaunchKernelGGL(gen_mul_kernel<G1>, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, s, (const Fr*)d_scalars, (uint32_t)n,
                           (const Affine<G1>*)tab.g1, (Xyzz<G1>*)ws);
        enqueue_affine<G1>(ws, (uint32_t)n, (uint8_t*)d_points, true, s);
    } else {
        hipLaunchKernelGGL(gen_mul_kernel<G2>, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, s, (const Fr*)d_scalars, (uint32_t)n,
                           (const Affine<G2>*)tab.g2, (Xyzz<G2>*)ws);
        enqueue_affine<G2>(ws, (uint32_t)n, (uint8_t*)d_points, true, s);
    }
    e = hipGetLastError();
    const hipError_t ef = hipFreeAsync(ws, s);
    if (e != hipSuccess) return fail(status, hip_err("launching the generator multiplications", e));
    if (ef != hipSuccess) return fail(status, hip_err("releasing the multiplication workspace", ef));
    set_ok(status);
    return 0;
}

int gwb_groth16_setup_phase_ms(float* ms) { return g_phases.read(ms); }

}  // extern "C"
