// R1CS satisfaction check on gfx950: for every (witness row s, constraint j)
//     ok(s, j) <=> (sum_A a w) * (sum_B b w) - sum_C c w == 0 (mod r)
// with per-row results first_failed[s] (smallest failing original index) and n_failed[s].
//
// Exactness with one Montgomery product per general factor: coefficients are stored as c * R, so fr_mul(w, cR) = c * w
// for a canonical w and c * w * R for a Montgomery-form w, fully reduced either way; +1 / -1 factors add or subtract w
// itself.  The comparison is fr_mul(A, B) (= AB / R) against C / R (canonical rows: fr_mul(C, 1)) or against C
// (Montgomery rows: AB / R = ab * R = c * R).  An element at or above r in a row (not a field element; .wtns images are
// refused on the host) is reduced where it is added directly, so the result is still exact mod r.
//
// Lane mapping: a wavefront covers T rows x 64/T constraints (T a power of two in 1..64).  At T = 64 the constraint is
// wave-uniform: its factor stream and coefficients come through scalar loads, every lane gathers the 32 bytes of its own
// row.  At small T (T = 1: the single-file case) every lane walks a constraint of its own; the host buckets constraints
// by length so that the lanes of a wave do similar work.
#include <hip/hip_runtime.h>

#include <string.h>

#include <string>

#include "hip_util.hpp"
#include "lincomb.hpp"
#include "r1cs_internal.hpp"

using namespace cwc_r1cs;
using cwc::Fr;

namespace {

constexpr int WAVES_PER_BLOCK = 4;

template <int T>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void r1cs_check_kernel(
    const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ fac, const uint32_t* __restrict__ cidx,
    const Fr* __restrict__ coef, const uint32_t* __restrict__ perm, uint32_t n_constraints, const uint8_t* __restrict__ witness,
    uint32_t n_witness, uint32_t batch, uint32_t montgomery, uint32_t* __restrict__ first_failed, uint32_t* __restrict__ n_failed) {
    constexpr uint32_t G = 64 / T;  // constraints per wave step
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t set = blockIdx.x * T + lane % T;
    const bool set_ok = set < batch;
    if (!set_ok) set = batch - 1;  // (a duplicate of a real row; its result is dropped)
    const uint8_t* row = witness + (size_t)set * n_witness * 32;
    const uint32_t n_groups = (n_constraints + G - 1) / G;
    const Fr one{{1, 0, 0, 0, 0, 0, 0, 0}};
    for (uint32_t g = blockIdx.y * WAVES_PER_BLOCK + wave; g < n_groups; g += gridDim.y * WAVES_PER_BLOCK) {
        uint32_t c = g * G + lane / T;  // T = 64: wave-uniform
        const bool c_ok = c < n_constraints;
        if (!c_ok) c = n_constraints - 1;
        const uint32_t ka = rowptr[3 * c], kb = rowptr[3 * c + 1], kc = rowptr[3 * c + 2], ke = rowptr[3 * c + 3];
        const Fr a = lin_comb(fac, cidx, coef, ka, kb, row);
        const Fr b = ka == kb ? cwc::fr_zero() : lin_comb(fac, cidx, coef, kb, kc, row);  // (linear constraints: A, B empty)
        const Fr cc = lin_comb(fac, cidx, coef, kc, ke, row);
        const Fr lhs = cwc::fr_mul(a, b);
        const Fr rhs = montgomery ? cc : cwc::fr_mul(cc, one);
        if (!cwc::u256_eq(lhs, rhs) && set_ok && c_ok) {  // rare: failing sets only
            atomicMin(first_failed + set, perm[c]);
            atomicAdd(n_failed + set, 1u);
        }
    }
}

typedef void (*KernelFn)(const uint32_t*, const uint32_t*, const uint32_t*, const Fr*, const uint32_t*, uint32_t, const uint8_t*, uint32_t,
                         uint32_t, uint32_t, uint32_t*, uint32_t*);

KernelFn kernel_for(uint32_t t) {
    switch (t) {
        case 1: return r1cs_check_kernel<1>;
        case 2: return r1cs_check_kernel<2>;
        case 4: return r1cs_check_kernel<4>;
        case 8: return r1cs_check_kernel<8>;
        case 16: return r1cs_check_kernel<16>;
        case 32: return r1cs_check_kernel<32>;
        default: return r1cs_check_kernel<64>;
    }
}

}  // namespace

// Host helpers over a RowSystem, shared with qap.hip and msm.hip (declared in r1cs_internal.hpp).
namespace cwc_r1cs {

// rows per wave: the batch rounded up to a power of two, at most 64 (full waves of rows once there are 64 of them)
static uint32_t pick_tile_width(size_t batch) {
    uint32_t t = 1;
    while (t < 64 && t < batch) t <<= 1;
    return t;
}

const char* prefix_of(const RowSystem& s) { return s.stride == 3 ? "r1cs: " : "zkey: "; }

template <class V>
static bool upload(DeviceBuf& d, const V& v, std::string& err) {
    const hipError_t e = d.upload(v.data(), v.size() * sizeof(v[0]));
    if (e != hipSuccess) err = hip_err("uploading the constraint arrays", e);
    return e == hipSuccess;
}

bool ensure_device(RowSystem& s, int home, std::string& err) {
    const std::string who = prefix_of(s);
    int dev = -1, n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        err = who + "no HIP device (the kernels run on the GPU only)";
        return false;
    }
    if (hipGetDevice(&dev) != hipSuccess) {
        err = who + "hipGetDevice failed";
        return false;
    }
    if (s.device >= 0) home = s.device;
    if (home >= 0 && dev != home) {
        err = who + "the handle's arrays live on device " + std::to_string(home) + ", the current device is " + std::to_string(dev);
        return false;
    }
    if (s.device >= 0) return true;
    DeviceBuf up[5];  // the row system gets all five or none
    if (!upload(up[0], s.rowptr, err) || !upload(up[1], s.fac, err) || !upload(up[2], s.cidx, err) || !upload(up[3], s.coef, err) ||
        !upload(up[4], s.perm, err))
        return false;
    DeviceBuf* dst[5] = {&s.d_rowptr, &s.d_fac, &s.d_cidx, &s.d_coef, &s.d_perm};
    for (int i = 0; i < 5; ++i) *dst[i] = std::move(up[i]);
    s.device = dev;
    return true;
}

bool check_args(const RowSystem& s, size_t n_witness, size_t batch, std::string& err) {
    if (n_witness != s.n_wires) {
        err = s.stride == 3 ? "r1cs: the witness has " + std::to_string(n_witness) + " elements, the circuit " + std::to_string(s.n_wires) + " wires"
                            : "zkey: the witness has " + std::to_string(n_witness) + " elements, the key nVars = " + std::to_string(s.n_wires);
        return false;
    }
    if (batch > 0xffffffffull) {
        err = std::string(prefix_of(s)) + "batch above 2^32 - 1";
        return false;
    }
    return true;
}

int cu_count(int device) {
    int cus = 0;
    return hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0 ? cus : 256;
}

bool eval_grid(const RowSystem& s, uint64_t rows, int cus, int waves, EvalGrid& g, std::string& err) {
    const uint32_t t = s.tile_width ? s.tile_width : pick_tile_width(rows);
    const uint32_t per_wave = 64 / t;
    const uint64_t n_groups = (s.n_rows + (uint64_t)per_wave - 1) / per_wave, tiles = (rows + t - 1) / t;
    // about eight blocks (32 waves) per CU in all, each wave striding over the constraint groups
    const uint64_t want_y = std::max<uint64_t>(1, (uint64_t)cus * 8 / std::max<uint64_t>(tiles, 1));
    const uint64_t gy = std::min<uint64_t>({want_y, (n_groups + waves - 1) / waves, 65535});
    if (tiles > 0x7fffffffull) {
        err = std::string(prefix_of(s)) + "batch too large for one launch";
        return false;
    }
    g = EvalGrid{t, (uint32_t)tiles, (uint32_t)gy};
    return true;
}

int fail(gw_status_t* st, const std::string& msg) {
    set_status(st, msg);
    return 1;
}

static bool parse_fail(std::string& err, const std::string& msg) {
    err = msg;
    return false;
}

bool parse_wtns(const void* wtns, size_t len, const uint8_t** values_out, uint64_t* n_wit_out, std::string& err) {
    // "wtns", u32 version (1 or 2), u32 nSections, sections {u32 type, u64 size}: 1 = {u32 n8, prime, u32 nWitness}, 2 = the values
    const uint8_t* p = (const uint8_t*)wtns;
    if (len < 12 || memcmp(p, "wtns", 4) != 0) return parse_fail(err, "wtns: bad magic (not a .wtns image)");
    uint32_t version, nsec;
    memcpy(&version, p + 4, 4);
    memcpy(&nsec, p + 8, 4);
    if (version != 1 && version != 2) return parse_fail(err, "wtns: unsupported version " + std::to_string(version));
    size_t off = 12;
    const uint8_t* values = nullptr;
    uint64_t values_size = 0, n_wit = 0;
    bool have_hdr = false;
    for (uint32_t i = 0; i < nsec; ++i) {
        if (len - off < 12) return parse_fail(err, "wtns: truncated section header");
        uint32_t type;
        uint64_t size;
        memcpy(&type, p + off, 4);
        memcpy(&size, p + off + 4, 8);
        off += 12;
        if (size > len - off) return parse_fail(err, "wtns: truncated section " + std::to_string(type));
        if (type == 1) {
            if (have_hdr) return parse_fail(err, "wtns: duplicate header section");
            if (size != 40) return parse_fail(err, "wtns: header section size " + std::to_string(size) + " (40 expected)");
            uint32_t n8, nw;
            memcpy(&n8, p + off, 4);
            Fr prime;
            memcpy(prime.v, p + off + 4, 32);
            memcpy(&nw, p + off + 36, 4);
            if (n8 != 32 || !cwc::u256_eq(prime, cwc::fr_p())) return parse_fail(err, "wtns: field is not BN254's r");
            n_wit = nw;
            have_hdr = true;
        } else if (type == 2) {
            if (values) return parse_fail(err, "wtns: duplicate witness section");
            values = p + off;
            values_size = size;
        }
        off += size;
    }
    if (off != len) return parse_fail(err, "wtns: " + std::to_string(len - off) + " trailing bytes");
    if (!have_hdr || !values) return parse_fail(err, "wtns: missing header or witness section");
    if (values_size != n_wit * 32) return parse_fail(err, "wtns: witness section size disagrees with nWitness x 32");
    for (uint64_t i = 0; i < n_wit; ++i) {
        Fr v;
        memcpy(v.v, values + 32 * i, 32);
        if (!cwc::u256_lt(v, cwc::fr_p())) return parse_fail(err, "wtns: witness element " + std::to_string(i) + " is not below r");
    }
    *values_out = values;
    *n_wit_out = n_wit;
    return true;
}

}  // namespace cwc_r1cs

namespace {

// enqueue: result initialisation + the check kernel on `stream`
bool enqueue(gwb_r1cs* r, const void* d_witness, size_t batch, uint32_t form, uint32_t* d_first, uint32_t* d_nfail, hipStream_t stream,
             std::string& err) {
    hipError_t e = hipMemsetAsync(d_first, 0xff, batch * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_nfail, 0, batch * 4, stream);
    if (e != hipSuccess) {
        err = hip_err("clearing the results", e);
        return false;
    }
    const RowSystem& sys = r->sys;
    if (sys.n_rows == 0) return true;
    EvalGrid g;
    if (!eval_grid(sys, batch, cu_count(sys.device), WAVES_PER_BLOCK, g, err)) return false;
    hipLaunchKernelGGL(kernel_for(g.t), dim3(g.tiles, g.gy), dim3(64 * WAVES_PER_BLOCK), 0, stream, sys.d_rowptr.as<const uint32_t>(),
                       sys.d_fac.as<const uint32_t>(), sys.d_cidx.as<const uint32_t>(), sys.d_coef.as<const Fr>(), sys.d_perm.as<const uint32_t>(), sys.n_rows,
                       (const uint8_t*)d_witness, sys.n_wires, (uint32_t)batch, form == GWB_FORM_MONTGOMERY ? 1u : 0u, d_first, d_nfail);
    e = hipGetLastError();
    if (e != hipSuccess) {
        err = hip_err("launching the check kernel", e);
        return false;
    }
    return true;
}

// host rows -> device -> results back; synchronous
int check_host(gwb_r1cs* r, const void* witness, size_t n_witness, size_t batch, uint32_t* first, uint32_t* nfail, gw_status_t* status) {
    std::string err;
    if (!check_args(r->sys, n_witness, batch, err)) return fail(status, err);
    if (batch == 0) {
        set_ok(status);
        return 0;
    }
    if (!ensure_device(r->sys, -1, err)) return fail(status, err);
    const size_t wbytes = batch * n_witness * 32;
    auto run = [&](unsigned char* const* d, hipStream_t s, std::string& err) {  // d[1]: first_failed, n_failed
        return enqueue(r, d[0], batch, GWB_FORM_CANONICAL, (uint32_t*)d[1], (uint32_t*)d[1] + batch, s, err);
    };
    if (!run_staged({wbytes, batch * 8}, {{witness, wbytes, 0, 0}}, {{first, batch * 4, 1, 0}, {nfail, batch * 4, 1, batch * 4}}, "staging the witness rows",
                    "running the check", run, err))
        return fail(status, err);
    set_ok(status);
    return 0;
}

}  // namespace

extern "C" {

void gwb_r1cs_free(gwb_r1cs_t* r) { delete r; }  // (the owners in it free what is on the device, with that device current)

int gwb_r1cs_check_batch_device(gwb_r1cs_t* r, const void* d_witness, size_t n_witness, size_t batch, uint32_t form, uint32_t* d_first_failed,
                                uint32_t* d_n_failed, void* hip_stream, gw_status_t* status) {
    if (!r || (batch && (!d_witness || !d_first_failed || !d_n_failed))) return fail(status, "gwb_r1cs_check_batch_device: NULL argument");
    if (form != GWB_FORM_CANONICAL && form != GWB_FORM_MONTGOMERY) return fail(status, "gwb_r1cs_check_batch_device: unknown form " + std::to_string(form));
    std::string err;
    if (!check_args(r->sys, n_witness, batch, err)) return fail(status, err);
    if (batch == 0) {
        set_ok(status);
        return 0;
    }
    if (!ensure_device(r->sys, -1, err) || !enqueue(r, d_witness, batch, form, d_first_failed, d_n_failed, (hipStream_t)hip_stream, err))
        return fail(status, err);
    set_ok(status);
    return 0;
}

int gwb_r1cs_check_batch_host(gwb_r1cs_t* r, const void* witness, size_t n_witness, size_t batch, uint32_t* first_failed, uint32_t* n_failed,
                              gw_status_t* status) {
    if (!r || (batch && (!witness || !first_failed || !n_failed))) return fail(status, "gwb_r1cs_check_batch_host: NULL argument");
    return check_host(r, witness, n_witness, batch, first_failed, n_failed, status);
}

int gwb_r1cs_check_wtns(gwb_r1cs_t* r, const void* wtns, size_t len, uint32_t* first_failed, uint32_t* n_failed, gw_status_t* status) {
    if (!r || !wtns || !first_failed || !n_failed) return fail(status, "gwb_r1cs_check_wtns: NULL argument");
    const uint8_t* values = nullptr;
    uint64_t n_wit = 0;
    std::string err;
    if (!parse_wtns(wtns, len, &values, &n_wit, err)) return fail(status, err);
    return check_host(r, values, n_wit, 1, first_failed, n_failed, status);
}

}  // extern "C"
