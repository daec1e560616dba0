// Groth16 verifier on gfx950 (include/graph_witness_groth16_verify.h has the definition), one thread per row and phase:
//
//   vkx_kernel       vk_x partial sums: one thread per (row, group of VKX_GROUP signals), Straus over 4-bit windows with the
//                    key's tables d IC_i (d = 1 .. 15, affine, built on the host at load)
//   check_kernel     per row: signal range (PUBLIC), coordinates and curves (POINT), [r] B = O (SUBGROUP); vk_x = IC_0 + the
//                    partials, made affine; the row's Miller-loop points A, B, -vk_x, -C in Montgomery form
//   miller_kernel    per row: one multi-Miller loop over (A, B) with B's lines formed on the fly and (-vk_x, gamma2),
//                    (-C, delta2) with the key's prepared lines; rows that already failed are skipped
//   easy_kernel      per row: the final exponentiation's easy part (its Fq12 inversion alone in a kernel)
//   final_kernel     per row: the hard part, compared with the key's e(alpha1, beta2) (or, for the pairing aid,
//                    written out as GT bytes): a 330-op program over one register accumulator and slots in a coalesced buffer
//
// Per key, once: lines_kernel prepares the lines of gamma2 and delta2 (fq12_gfx950.hpp's schedule), and e(alpha1, beta2)
// goes through the pairing aid's path.  Everything is per-thread Fq12 arithmetic (fq12_gfx950.hpp); the Miller loop and the
// final exponentiation walk schedules (MillerSched, FxProg) so each Fq12 primitive has one call site, which keeps the code
// small and out of compiler scratch.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/graph_witness_groth16_verify.h"
#include "fq12_gfx950.hpp"
#include "groth16_internal.hpp"
#include "hip_util.hpp"

using namespace cwc_r1cs;
using namespace cwc_g16;
using cwc::Fr;

namespace {

constexpr uint32_t THREADS = 64;
constexpr uint32_t VKX_GROUP = 8;   // signals per vk_x thread
constexpr uint32_t TAB = 15;        // table entries d IC_i, d = 1 .. 15
constexpr size_t KEY_BYTES = 64 + 3 * 128;

// the Miller-loop points of a row (Montgomery; (0, 0) = infinity)
struct RowPts {
    A1 a, vx, c;  // A, -vk_x, -C
    A2 b;
};

// ---- device ---------------------------------------------------------------------------------------------------------------
__constant__ MillerSched c_sched = miller_sched();
__constant__ FxProg c_fx = fx_prog();

__global__ __launch_bounds__(THREADS) void lines_kernel(A2 q0, A2 q1, Line* __restrict__ out) {
    const uint32_t t = threadIdx.x;
    if (t >= 2) return;
    const A2 q = t ? q1 : q0;
    if (affine_is_inf(q)) return;
    Line* o = out + (size_t)t * N_LINES;
    G2Proj T{q.x, q.y, fq2_one()};
    for (uint32_t k = 0; k < N_LINES; ++k) o[k] = miller_step(c_sched.kind[k], T, q.x, q.y);
}

__global__ __launch_bounds__(THREADS) void vkx_kernel(const uint8_t* __restrict__ pub, uint32_t npub, uint32_t rows, uint32_t n_groups,
                                                      const A1* __restrict__ tab, P1* __restrict__ part) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)rows * n_groups) return;
    const uint32_t row = (uint32_t)(t / n_groups), g = (uint32_t)(t % n_groups);
    const uint32_t i0 = g * VKX_GROUP, i1 = std::min(i0 + VKX_GROUP, npub);
    const uint32_t* s = reinterpret_cast<const uint32_t*>(pub + (size_t)row * npub * 32);
    P1 acc = xyzz_inf<G1>();
    for (int win = 63; win >= 0; --win) {
        for (int d = 0; d < 4; ++d) acc = xyzz_dbl(acc);
        const uint32_t w = (uint32_t)win >> 3, sh = 4u * ((uint32_t)win & 7u);
        for (uint32_t i = i0; i < i1; ++i) {
            const uint32_t dig = (s[(size_t)i * 8 + w] >> sh) & 15u;
            if (dig == 0) continue;
            const A1 b = tab[(size_t)i * TAB + dig - 1];
            if (!affine_is_inf(b)) acc = xyzz_add_affine(acc, b);
        }
    }
    part[t] = acc;
}

__global__ __launch_bounds__(THREADS) void check_kernel(const uint8_t* __restrict__ proofs, const uint8_t* __restrict__ pub, uint32_t npub,
                                                        uint32_t rows, A1 ic0, const P1* __restrict__ part, uint32_t n_groups,
                                                        RowPts* __restrict__ pts, uint32_t* __restrict__ status) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    uint32_t st = GWB_G16V_VALID;
    const uint8_t* s = pub + (size_t)row * npub * 32;
    for (uint32_t i = 0; i < npub; ++i)
        if (!cwc::u256_lt(rd_fq(s + (size_t)i * 32), cwc::fr_p())) st = GWB_G16V_PUBLIC;
    const uint8_t* p = proofs + (size_t)row * GWB_GROTH16_PROOF_BYTES;
    RowPts r;
    bool ok = get_coords<G1>(p, true, r.a.x, r.a.y);
    ok = cwc::both(ok, get_coords<G2>(p + 64, true, r.b.x, r.b.y));
    ok = cwc::both(ok, get_coords<G1>(p + 192, true, r.c.x, r.c.y));
    const bool a_inf = affine_is_inf(r.a), b_inf = affine_is_inf(r.b), c_inf = affine_is_inf(r.c);
    ok = cwc::both(ok, cwc::either(a_inf, on_curve<G1>(r.a, curve_b<G1>())));
    ok = cwc::both(ok, cwc::either(c_inf, on_curve<G1>(r.c, curve_b<G1>())));
    ok = cwc::both(ok, cwc::either(b_inf, on_curve<G2>(r.b, curve_b<G2>())));
    if (st == GWB_G16V_VALID && !ok) st = GWB_G16V_POINT;
    if (st == GWB_G16V_VALID && !b_inf && !xyzz_is_inf(xyzz_mul(from_affine(r.b), cwc::fr_p())))
        st = GWB_G16V_SUBGROUP;
    if (st == GWB_G16V_VALID) {
        P1 vx = from_affine(ic0);
        for (uint32_t g = 0; g < n_groups; ++g) vx = xyzz_add(vx, part[(size_t)row * n_groups + g]);
        r.vx = xyzz_to_affine(vx);
        r.vx.y = fq_neg(r.vx.y);  // (0, 0) stays (0, 0)
        r.c.y = fq_neg(r.c.y);
        pts[row] = r;
    }
    status[row] = st;
}

// Fq12 values of `rows` threads, word-interleaved: word k of slot s of row i at (s * 96 + k) * rows + i (coalesced).  The
// accesses are volatile so that the compiler neither forwards a spilled value nor keeps a reloaded one live in registers.
__device__ __forceinline__ void spill12(uint32_t* buf, uint32_t slot, uint32_t row, uint32_t rows, const Fq12& v) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&v);
    volatile uint32_t* b = buf;
#pragma unroll
    for (uint32_t k = 0; k < 96; ++k) b[((size_t)slot * 96 + k) * rows + row] = w[k];
}
__device__ __forceinline__ Fq12 fill12(const uint32_t* buf, uint32_t slot, uint32_t row, uint32_t rows) {
    Fq12 v;
    uint32_t* w = reinterpret_cast<uint32_t*>(&v);
    const volatile uint32_t* b = buf;
#pragma unroll
    for (uint32_t k = 0; k < 96; ++k) w[k] = b[((size_t)slot * 96 + k) * rows + row];
    return v;
}
// a value of global memory read where it is used (volatile: not hoisted out of a loop, not kept live)
template <class X>
__device__ __forceinline__ X ld_v(const X* p) {
    static_assert(sizeof(X) % 16 == 0, "whole uint4s");
    X v;
    uint4* w = reinterpret_cast<uint4*>(&v);
    const volatile uint4* s = reinterpret_cast<const volatile uint4*>(p);
#pragma unroll
    for (uint32_t k = 0; k < sizeof(X) / 16; ++k) {
        const uint4 t{s[k].x, s[k].y, s[k].z, s[k].w};
        w[k] = t;
    }
    return v;
}

// f of one row: lines of (A, B) on the fly, of (-vk_x, gamma2) and (-C, delta2) from `lines` (nullptr: the pair (A, B) only)
__global__ __launch_bounds__(THREADS) void miller_kernel(const RowPts* __restrict__ pts, uint32_t rows, const uint32_t* __restrict__ status,
                                                         const Line* __restrict__ lines, uint32_t fixed_inf, Fq12* __restrict__ fout) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows || (status && status[row] != GWB_G16V_VALID)) return;
    const RowPts* rp = pts + row;
    const RowPts r0 = *rp;
    const bool use_ab = !cwc::either(affine_is_inf(r0.a), affine_is_inf(r0.b));
    const bool use_g = lines && !(fixed_inf & 1u) && !affine_is_inf(r0.vx);
    const bool use_d = lines && !(fixed_inf & 2u) && !affine_is_inf(r0.c);
    Fq12 f = fq12_one();
    G2Proj T{r0.b.x, r0.b.y, fq2_one()};
    for (uint32_t k = 0; k < N_LINES; ++k) {
        const uint32_t kind = c_sched.kind[k];
        if (kind == 0) f = fq12_sqr(f);
        const A2 b = ld_v(&rp->b);
        const Line l = miller_step(kind, T, b.x, b.y);
#pragma unroll 1
        for (uint32_t j = 0; j < 3; ++j) {  // (A, B), (-vk_x, gamma2), (-C, delta2): one line product site
            const bool use = j == 0 ? use_ab : j == 1 ? use_g : use_d;
            if (!use) continue;
            const Line lj = j == 0 ? l : ld_v(lines + (j - 1) * N_LINES + k);
            const A1 p = ld_v(j == 0 ? &rp->a : j == 1 ? &rp->vx : &rp->c);
            f = fq12_mul_line_at(f, lj, p.x, p.y);
        }
    }
    fout[row] = f;
}

// fin[row] <- its easy part (rows not VALID are skipped when status is given)
__global__ __launch_bounds__(THREADS) void easy_kernel(Fq12* __restrict__ fin, uint32_t rows, const uint32_t* __restrict__ status) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows || (status && status[row] != GWB_G16V_VALID)) return;
    const Fq12 e = final_exp_easy([&] { return ld_v(fin + row); });
    fin[row] = e;
}

// ab != nullptr: status[row] = EQUATION unless f^e == *ab (rows not VALID are skipped); else gt[row] = f^e, canonical bytes
__global__ __launch_bounds__(THREADS) void final_kernel(const Fq12* __restrict__ fin, uint32_t rows, const Fq12* __restrict__ ab,
                                                        uint32_t* __restrict__ status, uint32_t* __restrict__ spill, uint8_t* __restrict__ gt) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows || (ab && status[row] != GWB_G16V_VALID)) return;
    const Fq12 e = final_exp_run(c_fx, ld_v(fin + row), [&](uint32_t s, const Fq12& v) { spill12(spill, s, row, rows, v); },
                                 [&](uint32_t s) { return fill12(spill, s, row, rows); });
    if (ab) {
        if (!fq12_eq(e, *ab)) status[row] = GWB_G16V_EQUATION;
        return;
    }
    const Fq* c = reinterpret_cast<const Fq*>(&e);
    Fq* o = reinterpret_cast<Fq*>(gt + (size_t)row * GWB_GT_BYTES);
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = fq_from_mont(c[k]);  // constant indices: e stays in registers
}

// canonical pairs -> RowPts (A = P, B = Q; no fixed pairs)
__global__ __launch_bounds__(THREADS) void pairs_kernel(const uint8_t* __restrict__ g1, const uint8_t* __restrict__ g2, uint32_t n,
                                                        RowPts* __restrict__ pts) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    RowPts r;  // coordinates that are not below q are taken as they reduce
    get_coords<G1>(g1 + (size_t)i * G1_BYTES, true, r.a.x, r.a.y);
    get_coords<G2>(g2 + (size_t)i * G2_BYTES, true, r.b.x, r.b.y);
    r.vx = r.c = A1{fq_zero(), fq_zero()};
    pts[i] = r;
}

// pairing aid path on a workspace of n RowPts, n Fq12 and FX_SLOTS n spill slots
bool enqueue_pairing(const uint8_t* g1, const uint8_t* g2, uint32_t n, uint8_t* gt, void* ws, hipStream_t s, std::string& err) {
    RowPts* pts = (RowPts*)ws;
    Fq12* f = (Fq12*)(pts + n);
    uint32_t* sp = (uint32_t*)(f + n);
    hipLaunchKernelGGL(pairs_kernel, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, s, g1, g2, n, pts);
    hipLaunchKernelGGL(miller_kernel, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, s, pts, n, (const uint32_t*)nullptr, (const Line*)nullptr, 0u, f);
    hipLaunchKernelGGL(easy_kernel, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, s, f, n, (const uint32_t*)nullptr);
    hipLaunchKernelGGL(final_kernel, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, s, f, n, (const Fq12*)nullptr, (uint32_t*)nullptr, sp, gt);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        err = hip_err("launching the pairing kernels", e);
        return false;
    }
    return true;
}

size_t pairing_ws(uint64_t n) { return n * (sizeof(RowPts) + sizeof(Fq12) + FX_SLOTS * sizeof(Fq12)); }

}  // namespace

// ---- host: the key ----------------------------------------------------------------------------------------------------------
struct gwb_g16vk {
    uint32_t n_public = 0;
    std::vector<uint8_t> points;  // canonical, gwb_g16vk_load's layout
    A1 ic0{};
    std::vector<A1> tab;          // [nPublic][15] d IC_i (Montgomery, affine)
    A2 gamma2{}, delta2{};
    bool ab_ready = false;
    uint8_t ab[GWB_GT_BYTES] = {};
    int device = -1;
    DeviceBuf d_lines, d_tab, d_ab;  // Line[2 N_LINES], A1[tab.size()], one Fq12: all three (ensure_key) or none
    Workspace ws;
};

namespace {

struct Fail {
    std::string msg;
};

// a canonical point at p -> Montgomery affine; refusals name the point
template <class T>
Affine<T> key_point(const uint8_t* p, const std::string& what) {
    Affine<T> a;
    const PointFault f = get_point<T>(p, true, a);
    if (f == PointFault::COORDINATE) throw Fail{"verifying key: " + what + " has a coordinate >= q"};
    if (f == PointFault::CURVE) throw Fail{"verifying key: " + what + (std::is_same<T, G2>::value ? " is not on the G2 twist curve" : " is not on the G1 curve")};
    return a;
}
// a G2 point of the key must also have order r: [r] P = O
A2 key_point_g2(const uint8_t* p, const std::string& what) {
    const A2 a = key_point<G2>(p, what);
    if (!xyzz_is_inf(xyzz_mul(from_affine(a), cwc::fr_p()))) throw Fail{"verifying key: " + what + " is not in the order-r subgroup of G2"};
    return a;
}

void load_key(const uint8_t* d, size_t len, uint32_t n_public, gwb_g16vk& k) {
    const size_t want = KEY_BYTES + 64 * ((size_t)n_public + 1);
    if (n_public > (1u << 24) || len != want) {
        const long long n_ic = len >= KEY_BYTES && (len - KEY_BYTES) % 64 == 0 ? (long long)((len - KEY_BYTES) / 64) : -1;
        throw Fail{"verifying key: " + (n_ic >= 0 ? std::to_string(n_ic) + " IC points" : std::to_string(len) + " bytes") + " for nPublic " +
                   std::to_string(n_public) + " (" + std::to_string((unsigned long long)n_public + 1) + " IC points, " + std::to_string(want) +
                   " bytes expected)"};
    }
    k.n_public = n_public;
    k.points.assign(d, d + len);
    key_point<G1>(d, "alpha1");
    key_point_g2(d + 64, "beta2");
    k.gamma2 = key_point_g2(d + 192, "gamma2");
    k.delta2 = key_point_g2(d + 320, "delta2");
    k.ic0 = key_point<G1>(d + KEY_BYTES, "IC[0]");
    k.tab.resize((size_t)n_public * TAB);
    for (uint32_t i = 0; i < n_public; ++i) {
        const A1 p = key_point<G1>(d + KEY_BYTES + 64 * ((size_t)i + 1), "IC[" + std::to_string(i + 1) + "]");
        P1 acc = xyzz_inf<G1>();
        for (uint32_t m = 0; m < TAB; ++m) {
            acc = affine_is_inf(p) ? acc : xyzz_add_affine(acc, p);
            k.tab[(size_t)i * TAB + m] = xyzz_to_affine(acc);
        }
    }
}

// the key's device data on the current device (first call; synchronous): lines of gamma2 and delta2, the IC tables,
// e(alpha1, beta2) (through the pairing path) in canonical bytes and in Montgomery form
bool ensure_key(gwb_g16vk* k, std::string& err) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && k->d_lines) {
        if (dev == k->device) return true;
        err = "groth16 verify: the key's data live on device " + std::to_string(k->device) + ", the current device is " + std::to_string(dev);
        return false;
    }
    Stream s;
    DeviceBuf lines, tab, ab;  // the key gets all three or none
    if (e == hipSuccess) e = s.create();
    if (e == hipSuccess) e = lines.alloc(2 * N_LINES * sizeof(Line));
    if (e == hipSuccess) e = tab.alloc(k->tab.size() * sizeof(A1));
    if (e == hipSuccess) e = ab.alloc(sizeof(Fq12));
    if (e == hipSuccess && !k->tab.empty()) e = hipMemcpyAsync(tab.as(), k->tab.data(), k->tab.size() * sizeof(A1), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(lines_kernel, dim3(1), dim3(THREADS), 0, s, k->gamma2, k->delta2, lines.as<Line>());
        e = hipGetLastError();
    }
    if (e == hipSuccess && !k->ws.ensure(64 + 128 + GWB_GT_BYTES + pairing_ws(1), "allocating the verifier workspace", err)) return false;
    uint8_t* ws = k->ws.as<uint8_t>();
    if (e == hipSuccess) e = hipMemcpyAsync(ws, k->points.data(), 64, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(ws + 64, k->points.data() + 64, 128, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && !enqueue_pairing(ws, ws + 64, 1, ws + 192, ws + 192 + GWB_GT_BYTES, s, err)) {
        (void)hipStreamSynchronize(s);
        return false;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(k->ab, ws + 192, GWB_GT_BYTES, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) {
        Fq12 m;
        Fq* c = reinterpret_cast<Fq*>(&m);
        for (int i = 0; i < 12; ++i) c[i] = fq_to_mont(rd_fq(k->ab + 32 * i));
        e = hipMemcpy(ab.as(), &m, sizeof m, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        err = hip_err("preparing the verifying key on the device", e);
        return false;
    }
    k->d_lines = std::move(lines);
    k->d_tab = std::move(tab);
    k->d_ab = std::move(ab);
    k->device = dev;
    k->ab_ready = true;
    return true;
}

bool enqueue_verify(gwb_g16vk* k, const uint8_t* d_proofs, const uint8_t* d_pub, uint64_t batch, uint32_t* d_status, hipStream_t s,
                    std::string& err) {
    if (!ensure_key(k, err)) return false;
    const uint32_t n = (uint32_t)batch, npub = k->n_public, n_groups = (npub + VKX_GROUP - 1) / VKX_GROUP;
    const size_t part_bytes = (size_t)batch * n_groups * sizeof(P1);
    const size_t bytes = part_bytes + batch * (sizeof(RowPts) + sizeof(Fq12) + FX_SLOTS * sizeof(Fq12)) + 256;
    if (!k->ws.ensure(bytes, "allocating the verifier workspace", err)) return false;
    P1* part = k->ws.as<P1>();
    RowPts* pts = (RowPts*)(k->ws.as<uint8_t>() + ((part_bytes + 255) & ~(size_t)255));
    Fq12* f = (Fq12*)(pts + batch);
    uint32_t* sp = (uint32_t*)(f + batch);
    if (n_groups)
        hipLaunchKernelGGL(vkx_kernel, dim3(blocks_for((uint64_t)n * n_groups, THREADS)), dim3(THREADS), 0, s, d_pub, npub, n, n_groups, k->d_tab.as<const A1>(), part);
    hipLaunchKernelGGL(check_kernel, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, s, d_proofs, d_pub, npub, n, k->ic0, part, n_groups, pts, d_status);
    const uint32_t fixed_inf = (affine_is_inf(k->gamma2) ? 1u : 0u) | (affine_is_inf(k->delta2) ? 2u : 0u);
    hipLaunchKernelGGL(miller_kernel, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, s, pts, n, d_status, k->d_lines.as<const Line>(), fixed_inf, f);
    hipLaunchKernelGGL(easy_kernel, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, s, f, n, (const uint32_t*)d_status);
    hipLaunchKernelGGL(final_kernel, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, s, f, n, k->d_ab.as<const Fq12>(), d_status, sp, (uint8_t*)nullptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        err = hip_err("launching the verifier kernels", e);
        return false;
    }
    return true;
}

int make_key(const uint8_t* d, size_t len, uint32_t n_public, gwb_g16vk_t** out, gw_status_t* status) {
    *out = nullptr;
    gwb_g16vk* k = new gwb_g16vk();
    try {
        load_key(d, len, n_public, *k);
    } catch (const Fail& f) {
        delete k;
        return fail(status, f.msg);
    } catch (const std::bad_alloc&) {
        delete k;
        return fail(status, "verifying key: out of host memory");
    }
    *out = k;
    set_ok(status);
    return 0;
}

}  // namespace

extern "C" {

int gwb_g16vk_load(const void* points, size_t len, uint32_t n_public, gwb_g16vk_t** out, gw_status_t* status) {
    if (!out || (!points && len)) return fail(status, "gwb_g16vk_load: NULL argument");
    return make_key((const uint8_t*)points, len, n_public, out, status);
}

int gwb_g16vk_from_zkey(const gwb_zkey_t* z, gwb_g16vk_t** out, gw_status_t* status) {
    if (!z || !out) return fail(status, "gwb_g16vk_from_zkey: NULL argument");
    std::vector<uint8_t> pts;
    auto put = [&](const uint8_t* p, size_t words) {  // Montgomery ("LEM") -> canonical
        for (size_t i = 0; i < words; ++i) {
            const Fq c = fq_from_mont(rd_fq(p + 32 * i));
            pts.insert(pts.end(), (const uint8_t*)c.v, (const uint8_t*)c.v + 32);
        }
    };
    put(z->alpha1, 2);
    put(z->beta2, 4);
    put(z->gamma2, 4);
    put(z->delta2, 4);
    put(z->ic.data(), z->ic.size() / 32);
    return make_key(pts.data(), pts.size(), z->info.n_public, out, status);
}

int gwb_g16vk_info(const gwb_g16vk_t* vk, gwb_g16vk_info_t* info) {
    if (!vk || !info) return 1;
    info->n_public = vk->n_public;
    return 0;
}

int gwb_g16vk_points(const gwb_g16vk_t* vk, void* out, size_t len) {
    if (!vk || !out || len != vk->points.size()) return 1;
    memcpy(out, vk->points.data(), len);
    return 0;
}

int gwb_g16vk_alphabeta(gwb_g16vk_t* vk, void* gt, gw_status_t* status) {
    if (!vk || !gt) return fail(status, "gwb_g16vk_alphabeta: NULL argument");
    std::string err;
    if (!vk->ab_ready && !ensure_key(vk, err)) return fail(status, err);
    memcpy(gt, vk->ab, GWB_GT_BYTES);
    set_ok(status);
    return 0;
}

void gwb_g16vk_free(gwb_g16vk_t* vk) { delete vk; }

int gwb_groth16_verify_batch_device(gwb_g16vk_t* vk, const void* d_proofs, const void* d_public, size_t n_public, size_t batch, void* d_status,
                                    void* hip_stream, gw_status_t* status) {
    if (!vk || (batch && (!d_proofs || !d_status || (n_public && !d_public)))) return fail(status, "gwb_groth16_verify_batch_device: NULL argument");
    if (n_public != vk->n_public)
        return fail(status, "groth16 verify: " + std::to_string(n_public) + " public signals per row, the key has nPublic " + std::to_string(vk->n_public));
    if (batch > 0x7fffffffull) return fail(status, "groth16 verify: batch above 2^31 - 1");
    if (batch == 0) {
        set_ok(status);
        return 0;
    }
    std::string err;
    if (!enqueue_verify(vk, (const uint8_t*)d_proofs, (const uint8_t*)d_public, batch, (uint32_t*)d_status, (hipStream_t)hip_stream, err))
        return fail(status, err);
    set_ok(status);
    return 0;
}

int gwb_groth16_verify_batch_host(gwb_g16vk_t* vk, const void* proofs, const void* pub, size_t n_public, size_t batch, void* status_out,
                                  gw_status_t* status) {
    if (!vk || (batch && (!proofs || !status_out || (n_public && !pub)))) return fail(status, "gwb_groth16_verify_batch_host: NULL argument");
    if (n_public != vk->n_public)
        return fail(status, "groth16 verify: " + std::to_string(n_public) + " public signals per row, the key has nPublic " + std::to_string(vk->n_public));
    if (batch > 0x7fffffffull) return fail(status, "groth16 verify: batch above 2^31 - 1");
    if (batch == 0) {
        set_ok(status);
        return 0;
    }
    std::string err;
    const size_t pb = batch * GWB_GROTH16_PROOF_BYTES, sb = batch * n_public * 32;
    Carve c;  // one allocation: the proofs, the public signals, the statuses
    const size_t o_proofs = c.take(pb), o_pub = c.take(sb), o_st = c.take(batch * 4);
    auto run = [&](unsigned char* const* d, hipStream_t s, std::string& err) {
        return enqueue_verify(vk, d[0] + o_proofs, d[0] + o_pub, batch, (uint32_t*)(d[0] + o_st), s, err);
    };
    if (!run_staged({c.o}, {{proofs, pb, 0, o_proofs}, {pub, sb, 0, o_pub}}, {{status_out, batch * 4, 0, o_st}}, "staging the proofs", "running the verifier",
                    run, err))
        return fail(status, err);
    set_ok(status);
    return 0;
}

int gwb_bn254_pairing_batch_device(const void* d_g1, const void* d_g2, size_t n, void* d_gt, void* hip_stream, gw_status_t* status) {
    if (n && (!d_g1 || !d_g2 || !d_gt)) return fail(status, "gwb_bn254_pairing_batch_device: NULL argument");
    if (n > 0x7fffffffull) return fail(status, "gwb_bn254_pairing_batch_device: n above 2^31 - 1");
    if (n == 0) {
        set_ok(status);
        return 0;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    void* ws = nullptr;
    std::string err;
    hipError_t e = hipMallocAsync(&ws, pairing_ws(n), s);
    if (e != hipSuccess) return fail(status, hip_err("allocating the pairing workspace", e));
    const bool ok = enqueue_pairing((const uint8_t*)d_g1, (const uint8_t*)d_g2, (uint32_t)n, (uint8_t*)d_gt, ws, s, err);
    e = hipFreeAsync(ws, s);
    if (!ok) return fail(status, err);
    if (e != hipSuccess) return fail(status, hip_err("releasing the pairing workspace", e));
    set_ok(status);
    return 0;
}

}  // extern "C"
