// G2 subgroup membership of batches of twist points on gfx950 (g2_subgroup_gfx950.hpp has the criterion), for the points that
// reach the device after a coordinate and curve check alone: a `.zkey`'s beta2, gamma2, delta2 and section 7 (gwb_zkey_check_g2)
// and the G2 points a setup reads from a `.ptau` (gwb_ptau_check_g2); and the aid both go through
// (gwb_bn254_g2_check_batch_device, include/graph_witness_groth16_verify.h).  Opt-in everywhere: no loader calls it by itself.
//
//   g2_check_kernel<M>  one thread per point: coordinates below q and the curve equation (GWB_G16V_POINT), then membership
//                       (GWB_G16V_SUBGROUP) by the psi criterion (M = 0) or by [r] P = O (M = 1, the verifier's rule: cross-check
//                       and baseline).  Infinity is VALID.  Every lane of a wave walks the same chain of doublings and additions
//                       (the scalar's bits are constants); only invalid points and infinity leave early.
//   first_bad_kernel    the smallest 4 i + status over the nonzero statuses (atomicMin) and their count (atomicAdd)
//
// The file checks upload the points as stored, in pieces of CWC_G2_CHECK_CHUNK points (read at each call, default 2^18 = 32 MiB),
// on a stream of their own, and free everything before they return.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage for gfx950; every kernel: 0 bytes of scratch, 0 bytes of LDS):
//   g2_check_kernel<0>  106 SGPRs, 256 VGPRs + 125 AGPRs, 1 wave / SIMD
//   g2_check_kernel<1>  103 SGPRs, 256 VGPRs + 33 AGPRs, 1 wave / SIMD
//   first_bad_kernel    19 SGPRs, 4 VGPRs, 8 waves / SIMD
// The chain keeps the running left side and psi^k([x] P) (Xyzz<Fq2T>: 64 registers each) across an inlined addition with its
// own temporaries, which does not fit 256 registers: capped there (__launch_bounds__(64, 2)) the compiler spills 504 and 136
// bytes per lane, so the kernels run one wave per SIMD in the unified 512-register file, as setup_ptau.hip's G2 butterfly does,
// and one kernel holds the whole chain (no split into [x] P and the comparison is needed to stay out of scratch).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "../../include/graph_witness_groth16_ptau.h"
#include "../../include/graph_witness_groth16_verify.h"
#include "g2_subgroup_gfx950.hpp"
#include "groth16_internal.hpp"
#include "hip_util.hpp"
#include "ptau_internal.hpp"

using namespace cwc_r1cs;
using namespace cwc_g16;

namespace {

constexpr uint32_t THREADS = 64;
constexpr uint32_t REDUCE_THREADS = 256;
constexpr unsigned long long NONE_BAD = ~0ull;
constexpr uint64_t DEFAULT_CHUNK = 1ull << 18;

template <int METHOD>
__global__ __launch_bounds__(THREADS) void g2_check_kernel(const uint8_t* __restrict__ in, uint32_t n, uint32_t canonical,
                                                           uint32_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    A2 p;
    const bool in_range = get_coords<G2>(in + (size_t)i * G2_BYTES, canonical != 0, p.x, p.y);
    uint32_t st = GWB_G16V_VALID;
    if (!in_range) {
        st = GWB_G16V_POINT;
    } else if (!affine_is_inf(p)) {
        if (!on_curve<G2>(p, curve_b<G2>()))
            st = GWB_G16V_POINT;
        else if (!(METHOD == 0 ? g2_in_subgroup(p) : g2_in_subgroup_by_order(p)))
            st = GWB_G16V_SUBGROUP;
    }
    status[i] = st;
}

// *first = min over the nonzero status[i] of 4 i + status[i] (preset to NONE_BAD), *count += their number
__global__ __launch_bounds__(REDUCE_THREADS) void first_bad_kernel(const uint32_t* __restrict__ status, uint32_t n, unsigned long long* __restrict__ first,
                                                                   uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t st = status[i];
    if (st != 0) {
        atomicMin(first, 4ull * i + st);
        atomicAdd(count, 1u);
    }
}

bool enqueue_check(const uint8_t* d_points, uint32_t n, bool canonical, uint32_t method, uint32_t* d_status, hipStream_t s, std::string& err) {
    if (method == 0)
        hipLaunchKernelGGL(g2_check_kernel<0>, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, s, d_points, n, canonical ? 1u : 0u, d_status);
    else
        hipLaunchKernelGGL(g2_check_kernel<1>, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, s, d_points, n, canonical ? 1u : 0u, d_status);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        err = hip_err("launching the G2 subgroup check", e);
        return false;
    }
    return true;
}

uint64_t chunk_points() {
    const char* v = getenv("CWC_G2_CHECK_CHUNK");
    if (!v || !*v) return DEFAULT_CHUNK;
    const unsigned long long c = strtoull(v, nullptr, 10);
    return c >= 1 && c <= (1ull << 24) ? c : DEFAULT_CHUNK;
}

// The device side of one file check: a stream and the buffers of one piece, released with the object.
struct Checker {
    Stream s;
    DeviceBuf pts, status, res;  // res: [0] the smallest 4 i + status, [1]'s low word the count
    uint64_t chunk = 0;
    bool open(uint64_t largest, std::string& err) {
        chunk = std::max<uint64_t>(1, std::min(chunk_points(), largest));
        hipError_t e = s.create();
        if (e == hipSuccess) e = pts.alloc(chunk * G2_BYTES);
        if (e == hipSuccess) e = status.alloc(chunk * sizeof(uint32_t));
        if (e == hipSuccess) e = res.alloc(2 * sizeof(unsigned long long));
        if (e != hipSuccess) err = hip_err("allocating the G2 subgroup check's buffers", e);
        return e == hipSuccess;
    }
    // n points (Montgomery form, as the files store them) at host address p: the smallest index whose status is not VALID, that
    // status, and the number of such points (all pieces are checked, so the count is the array's).  statuses != nullptr: every
    // status, for a short array.
    bool run(const uint8_t* p, uint64_t n, uint64_t& first, uint32_t& first_status, uint64_t& count, uint32_t* statuses, std::string& err) {
        uint8_t* d_pts = pts.as<uint8_t>();
        uint32_t* d_status = status.as<uint32_t>();
        unsigned long long* d_res = res.as<unsigned long long>();
        first = NONE_BAD;
        first_status = GWB_G16V_VALID;
        count = 0;
        for (uint64_t at = 0; at < n; at += chunk) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - at);
            unsigned long long res[2] = {NONE_BAD, 0};
            hipError_t e = hipMemcpyAsync(d_pts, p + at * G2_BYTES, (size_t)m * G2_BYTES, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(d_res, res, sizeof res, hipMemcpyHostToDevice, s);
            if (e != hipSuccess) {
                err = hip_err("uploading G2 points", e);
                return false;
            }
            if (!enqueue_check(d_pts, m, false, 0, d_status, s, err)) return false;
            hipLaunchKernelGGL(first_bad_kernel, dim3(blocks_for(m, REDUCE_THREADS)), dim3(REDUCE_THREADS), 0, s, (const uint32_t*)d_status, m, d_res,
                               (uint32_t*)(d_res + 1));
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(res, d_res, sizeof res, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && statuses) e = hipMemcpyAsync(statuses + at, d_status, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) {
                err = hip_err("running the G2 subgroup check", e);
                return false;
            }
            if (res[0] != NONE_BAD && first == NONE_BAD) {
                first = at + (res[0] >> 2);
                first_status = (uint32_t)(res[0] & 3u);
            }
            count += (uint32_t)res[1];
        }
        return true;
    }
};

int check_zkey(gwb_zkey* z, gw_status_t* status) {
    const uint64_t n = z->info.n_vars;
    if (z->b2.size() != n * G2_BYTES) return fail(status, "zkey: section 7 (B2) does not hold nVars points");
    std::string err;
    Checker c;
    if (!c.open(std::max<uint64_t>(3, n), err)) return fail(status, err);
    uint8_t head[3 * G2_BYTES];
    memcpy(head, z->beta2, G2_BYTES);
    memcpy(head + G2_BYTES, z->gamma2, G2_BYTES);
    memcpy(head + 2 * G2_BYTES, z->delta2, G2_BYTES);
    uint64_t first, count;
    uint32_t st, sts[3];
    if (!c.run(head, 3, first, st, count, sts, err)) return fail(status, err);
    static const char* names[3] = {"beta2", "gamma2", "delta2"};
    for (int k = 0; k < 3; ++k)
        if (sts[k] != GWB_G16V_VALID) return fail(status, std::string("zkey: ") + names[k] + " is not in the order-r subgroup of G2");
    if (!c.run(z->b2.data(), n, first, st, count, nullptr, err)) return fail(status, err);
    if (first != NONE_BAD)
        return fail(status, "zkey: section 7 (B2) point " + std::to_string(first) + " is not in the order-r subgroup of G2 (" + std::to_string(count) +
                                " of " + std::to_string(n) + " points are not)");
    set_ok(status);
    return 0;
}

int check_ptau(const uint8_t* data, size_t len, uint32_t domain_power, uint32_t mode, gw_status_t* status) {
    std::string err;
    cwc_ptau::View view;
    cwc_ptau::Plan pl;
    if (!cwc_ptau::parse(data, len, view, err) || !cwc_ptau::plan(view, domain_power, mode, pl, err) || !cwc_ptau::check_header_points(pl, err))
        return fail(status, err);
    const uint64_t n = 1ull << pl.p;
    // the arrays in the order their faults are reported: section, index of the array's first point, points, address
    struct Arr {
        uint32_t section;
        uint64_t base, n;
        const uint8_t* p;
    };
    const Arr arrs[3] = {{6, 0, 1, pl.beta2}, {3, 0, pl.from_file ? 1 : n, pl.t2}, {13, n - 1, pl.from_file ? n : 0, pl.l2}};
    Checker c;
    if (!c.open(n, err)) return fail(status, err);
    for (const Arr& a : arrs) {
        if (a.n == 0) continue;
        uint64_t first, count;
        uint32_t st;
        if (!c.run(a.p, a.n, first, st, count, nullptr, err)) return fail(status, err);
        if (first == NONE_BAD) continue;
        // GWB_G16V_POINT: which of the loaders' two faults
        const PointFault fault = st == GWB_G16V_SUBGROUP ? PointFault::SUBGROUP : point_fault<G2>(a.p + first * G2_BYTES, false);
        return fail(status, cwc_ptau::point_message(a.section, a.base + first, fault, true));
    }
    set_ok(status);
    return 0;
}

}  // namespace

int cwc_ptau::check_g2_points(uint32_t section, uint64_t base, const uint8_t* p, uint64_t n, std::string& msg) {
    Checker c;
    uint64_t first, count;
    uint32_t st;
    if (!c.open(std::max<uint64_t>(1, n), msg) || !c.run(p, n, first, st, count, nullptr, msg)) return 2;
    if (first == NONE_BAD) return 0;
    const PointFault fault = st == GWB_G16V_SUBGROUP ? PointFault::SUBGROUP : point_fault<G2>(p + first * G2_BYTES, false);
    msg = point_message(section, base + first, fault, true);
    return 1;
}

extern "C" {

int gwb_bn254_g2_check_batch_device(const void* d_points, size_t n, uint32_t form, uint32_t method, void* d_status, void* hip_stream,
                                    gw_status_t* status) {
    if (form != GWB_FORM_CANONICAL && form != GWB_FORM_MONTGOMERY)
        return fail(status, "gwb_bn254_g2_check_batch_device: unknown form " + std::to_string(form));
    if (method > 1) return fail(status, "gwb_bn254_g2_check_batch_device: unknown method " + std::to_string(method) + " (0 = psi criterion, 1 = [r] P)");
    if (n && (!d_points || !d_status)) return fail(status, "gwb_bn254_g2_check_batch_device: NULL argument");
    if (n > 0x7fffffffull) return fail(status, "gwb_bn254_g2_check_batch_device: n above 2^31 - 1");
    if (n == 0) {
        set_ok(status);
        return 0;
    }
    std::string err;
    if (!enqueue_check((const uint8_t*)d_points, (uint32_t)n, form == GWB_FORM_CANONICAL, method, (uint32_t*)d_status, (hipStream_t)hip_stream, err))
        return fail(status, err);
    set_ok(status);
    return 0;
}

int gwb_zkey_check_g2(gwb_zkey_t* z, gw_status_t* status) {
    if (!z) return fail(status, "gwb_zkey_check_g2: NULL argument");
    try {
        return check_zkey(z, status);
    } catch (const std::bad_alloc&) {
        return fail(status, "zkey: out of host memory");
    }
}

int gwb_ptau_check_g2(const void* data, size_t len, uint32_t domain_power, uint32_t lagrange_mode, gw_status_t* status) {
    if (!data && len) return fail(status, "gwb_ptau_check_g2: NULL argument");
    try {
        return check_ptau((const uint8_t*)data, len, domain_power, lagrange_mode, status);
    } catch (const std::bad_alloc&) {
        return fail(status, "ptau: out of host memory");
    }
}

}  // extern "C"
