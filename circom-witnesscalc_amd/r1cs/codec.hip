// Compressed BN254 points, Groth16 proofs and verifying keys on gfx950 (include/graph_witness_groth16_compressed.h has the
// format; point_codec_gfx950.hpp the arithmetic), one thread per point in workgroups of one wave:
//
//   compress_points_kernel<C>     n stored points -> n encodings: no field product for canonical points, two conversions else
//   decompress_points_kernel<C>   n encodings -> n stored points and statuses; a G1 root is one exponentiation, a G2 root two
//                                 and an inversion (fq2_sqrt)
//   compress_proofs_kernel        [B][256] -> [B][128]
//   decompress_proofs_kernel      [B][128] -> [B][256]; a refused point writes GWB_G16V_POINT into its row's (zeroed) status
//   merge_status_kernel           the verifier's status of a row and its decoding status -> the row's status
//
// The proof kernels give every point a thread, not every proof, and keep the groups apart: the first blocks take the 2 B G1
// points (A and C of a row side by side), the blocks after them the B G2 points.  A G2 root costs about three G1 roots; with A,
// B and C in neighbouring lanes two lanes of three would wait for the third through two thirds of the kernel, and with a thread
// per proof every lane would run the three roots one after the other at a third of the parallelism.
//
// The compressed verify call decodes into a stream-ordered workspace and runs the unchanged verifier (verify.hip) through its
// public entry point on the raw proofs: rows that failed decoding reach it as points at infinity, and merge_status_kernel puts
// their POINT in place afterwards, behind PUBLIC as the documented rule order has it.  The compressed key is decoded on the host.
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/graph_witness_groth16_compressed.h"
#include "groth16_internal.hpp"
#include "hip_util.hpp"
#include "point_codec_gfx950.hpp"

using namespace cwc_r1cs;
using namespace cwc_g16;

static_assert(CODEC_OK == GWB_G16V_VALID && CODEC_POINT == GWB_G16V_POINT, "the codec's statuses are the verifier's");
static_assert(GWB_GROTH16_CPROOF_BYTES == 2 * G1_COMPRESSED_BYTES + G2_COMPRESSED_BYTES, "A, B, C");

namespace {

constexpr uint32_t THREADS = 64;
constexpr size_t KEY_FIXED = 64 + 3 * 128, CKEY_FIXED = 32 + 3 * 64 + 8;  // the bytes before IC: raw, compressed

// ---- device ---------------------------------------------------------------------------------------------------------------
template <class C>
__global__ __launch_bounds__(THREADS) void compress_points_kernel(const uint8_t* __restrict__ pts, uint32_t n, bool canonical,
                                                                  uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    point_encode<C>(pts + (size_t)i * C::POINT_BYTES, canonical, out + (size_t)i * C::COMPRESSED_BYTES);
}

template <class C>
__global__ __launch_bounds__(THREADS) void decompress_points_kernel(const uint8_t* __restrict__ in, uint32_t n, bool canonical,
                                                                    uint8_t* __restrict__ pts, uint32_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    status[i] = point_decode<C>(in + (size_t)i * C::COMPRESSED_BYTES, canonical, pts + (size_t)i * C::POINT_BYTES);
}

// blocks [0, g1_blocks): thread t < 2 rows is point A (t even) or C (t odd) of row t / 2; the blocks after: B of a row
__global__ __launch_bounds__(THREADS) void compress_proofs_kernel(const uint8_t* __restrict__ proofs, uint32_t rows, uint32_t g1_blocks,
                                                                  uint8_t* __restrict__ out) {
    if (blockIdx.x < g1_blocks) {
        const uint64_t t = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
        if (t >= 2ull * rows) return;
        const size_t row = (size_t)(t >> 1);
        const bool c = (t & 1u) != 0u;
        g1_encode(proofs + row * GWB_GROTH16_PROOF_BYTES + (c ? 192 : 0), true, out + row * GWB_GROTH16_CPROOF_BYTES + (c ? 96 : 0));
    } else {
        const uint64_t row = (uint64_t)(blockIdx.x - g1_blocks) * THREADS + threadIdx.x;
        if (row >= rows) return;
        g2_encode(proofs + (size_t)row * GWB_GROTH16_PROOF_BYTES + 64, true, out + (size_t)row * GWB_GROTH16_CPROOF_BYTES + 32);
    }
}

// the same mapping; status is zero on entry, and every refused point of a row writes the same GWB_G16V_POINT
__global__ __launch_bounds__(THREADS) void decompress_proofs_kernel(const uint8_t* __restrict__ in, uint32_t rows, uint32_t g1_blocks,
                                                                    uint8_t* __restrict__ proofs, uint32_t* __restrict__ status) {
    uint32_t st;
    size_t row;
    if (blockIdx.x < g1_blocks) {
        const uint64_t t = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
        if (t >= 2ull * rows) return;
        row = (size_t)(t >> 1);
        const bool c = (t & 1u) != 0u;
        st = g1_decode(in + row * GWB_GROTH16_CPROOF_BYTES + (c ? 96 : 0), true, proofs + row * GWB_GROTH16_PROOF_BYTES + (c ? 192 : 0));
    } else {
        row = (size_t)(blockIdx.x - g1_blocks) * THREADS + threadIdx.x;
        if (row >= rows) return;
        st = g2_decode(in + row * GWB_GROTH16_CPROOF_BYTES + 32, true, proofs + row * GWB_GROTH16_PROOF_BYTES + 64);
    }
    if (st != CODEC_OK) status[row] = GWB_G16V_POINT;
}

// PUBLIC, POINT, SUBGROUP, EQUATION: a refused encoding outranks everything but a public signal >= r
__global__ __launch_bounds__(THREADS) void merge_status_kernel(uint32_t* __restrict__ verify, const uint32_t* __restrict__ decode, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = verify[i];
    verify[i] = v == GWB_G16V_PUBLIC ? v : decode[i] != 0u ? GWB_G16V_POINT : v;
}

// ---- host -----------------------------------------------------------------------------------------------------------------
bool launched(const char* what, std::string& err) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) err = hip_err(what, e);
    return e == hipSuccess;
}

uint32_t g1_blocks_of(size_t batch) { return blocks_for(2ull * batch, THREADS); }

bool enqueue_compress_proofs(const uint8_t* d_proofs, size_t batch, uint8_t* d_out, hipStream_t s, std::string& err) {
    const uint32_t g1 = g1_blocks_of(batch);
    hipLaunchKernelGGL(compress_proofs_kernel, dim3(g1 + blocks_for(batch, THREADS)), dim3(THREADS), 0, s, d_proofs, (uint32_t)batch, g1, d_out);
    return launched("launching the proof compression kernel", err);
}

bool enqueue_decompress_proofs(const uint8_t* d_in, size_t batch, uint8_t* d_proofs, uint32_t* d_status, hipStream_t s, std::string& err) {
    const hipError_t e = hipMemsetAsync(d_status, 0, batch * 4, s);
    if (e != hipSuccess) {
        err = hip_err("clearing the decoding statuses", e);
        return false;
    }
    const uint32_t g1 = g1_blocks_of(batch);
    hipLaunchKernelGGL(decompress_proofs_kernel, dim3(g1 + blocks_for(batch, THREADS)), dim3(THREADS), 0, s, d_in, (uint32_t)batch, g1, d_proofs,
                       d_status);
    return launched("launching the proof decompression kernel", err);
}

// decode into a stream-ordered workspace, verify the raw proofs, merge the statuses
bool enqueue_verify_compressed(gwb_g16vk_t* vk, const uint8_t* d_cproofs, const void* d_public, size_t n_public, size_t batch, uint32_t* d_status,
                               hipStream_t s, std::string& err) {
    Carve c;
    const size_t o_proofs = c.take(batch * GWB_GROTH16_PROOF_BYTES), o_dec = c.take(batch * 4);
    void* ws = nullptr;
    hipError_t e = hipMallocAsync(&ws, c.o, s);
    if (e != hipSuccess) {
        err = hip_err("allocating the decoding workspace", e);
        return false;
    }
    uint8_t* raw = (uint8_t*)ws + o_proofs;
    uint32_t* dec = (uint32_t*)((uint8_t*)ws + o_dec);
    bool ok = enqueue_decompress_proofs(d_cproofs, batch, raw, dec, s, err);
    if (ok) {
        gw_status_t st = {OK, nullptr};
        if (gwb_groth16_verify_batch_device(vk, raw, d_public, n_public, batch, d_status, s, &st) != 0) {
            err = st.error_msg ? st.error_msg : "groth16 verify failed";
            gw_free_status(&st);
            ok = false;
        }
    }
    if (ok) {
        hipLaunchKernelGGL(merge_status_kernel, dim3(blocks_for(batch, THREADS)), dim3(THREADS), 0, s, d_status, (const uint32_t*)dec, (uint32_t)batch);
        ok = launched("launching the status merge kernel", err);
    }
    e = hipFreeAsync(ws, s);
    if (ok && e != hipSuccess) {
        err = hip_err("releasing the decoding workspace", e);
        ok = false;
    }
    return ok;
}

// the arguments of both compressed verify calls that need no device: empty when they are fine
std::string verify_args(const gwb_g16vk_t* vk, size_t n_public, size_t batch) {
    gwb_g16vk_info_t info{};
    gwb_g16vk_info(vk, &info);
    if (n_public != info.n_public)
        return "groth16 verify: " + std::to_string(n_public) + " public signals per row, the key has nPublic " + std::to_string(info.n_public);
    if (batch > 0x7fffffffull) return "groth16 verify: batch above 2^31 - 1";
    return "";
}

const char* group_form_error(uint32_t group, uint32_t form) {
    if (group != 1 && group != 2) return "group must be 1 (G1) or 2 (G2)";
    if (form != GWB_FORM_CANONICAL && form != GWB_FORM_MONTGOMERY) return "form must be GWB_FORM_CANONICAL or GWB_FORM_MONTGOMERY";
    return nullptr;
}

}  // namespace

extern "C" {

int gwb_bn254_compress_batch_device(const void* d_points, size_t n, uint32_t group, uint32_t form, void* d_out, void* hip_stream,
                                    gw_status_t* status) {
    if (const char* bad = group_form_error(group, form)) return fail(status, std::string("gwb_bn254_compress_batch_device: ") + bad);
    if (n && (!d_points || !d_out)) return fail(status, "gwb_bn254_compress_batch_device: NULL argument");
    if (n > 0x7fffffffull) return fail(status, "gwb_bn254_compress_batch_device: n above 2^31 - 1");
    if (n == 0) {
        set_ok(status);
        return 0;
    }
    const bool canonical = form == GWB_FORM_CANONICAL;
    const dim3 grid(blocks_for(n, THREADS)), block(THREADS);
    hipStream_t s = (hipStream_t)hip_stream;
    if (group == 1)
        hipLaunchKernelGGL(compress_points_kernel<G1Codec>, grid, block, 0, s, (const uint8_t*)d_points, (uint32_t)n, canonical, (uint8_t*)d_out);
    else
        hipLaunchKernelGGL(compress_points_kernel<G2Codec>, grid, block, 0, s, (const uint8_t*)d_points, (uint32_t)n, canonical, (uint8_t*)d_out);
    std::string err;
    if (!launched("launching the point compression kernel", err)) return fail(status, err);
    set_ok(status);
    return 0;
}

int gwb_bn254_decompress_batch_device(const void* d_in, size_t n, uint32_t group, uint32_t form, void* d_points, void* d_status, void* hip_stream,
                                      gw_status_t* status) {
    if (const char* bad = group_form_error(group, form)) return fail(status, std::string("gwb_bn254_decompress_batch_device: ") + bad);
    if (n && (!d_in || !d_points || !d_status)) return fail(status, "gwb_bn254_decompress_batch_device: NULL argument");
    if (n > 0x7fffffffull) return fail(status, "gwb_bn254_decompress_batch_device: n above 2^31 - 1");
    if (n == 0) {
        set_ok(status);
        return 0;
    }
    const bool canonical = form == GWB_FORM_CANONICAL;
    const dim3 grid(blocks_for(n, THREADS)), block(THREADS);
    hipStream_t s = (hipStream_t)hip_stream;
    if (group == 1)
        hipLaunchKernelGGL(decompress_points_kernel<G1Codec>, grid, block, 0, s, (const uint8_t*)d_in, (uint32_t)n, canonical, (uint8_t*)d_points,
                           (uint32_t*)d_status);
    else
        hipLaunchKernelGGL(decompress_points_kernel<G2Codec>, grid, block, 0, s, (const uint8_t*)d_in, (uint32_t)n, canonical, (uint8_t*)d_points,
                           (uint32_t*)d_status);
    std::string err;
    if (!launched("launching the point decompression kernel", err)) return fail(status, err);
    set_ok(status);
    return 0;
}

int gwb_groth16_proofs_compress_device(const void* d_proofs, size_t batch, void* d_out, void* hip_stream, gw_status_t* status) {
    if (batch && (!d_proofs || !d_out)) return fail(status, "gwb_groth16_proofs_compress_device: NULL argument");
    if (batch > 0x7fffffffull) return fail(status, "gwb_groth16_proofs_compress_device: batch above 2^31 - 1");
    std::string err;
    if (batch && !enqueue_compress_proofs((const uint8_t*)d_proofs, batch, (uint8_t*)d_out, (hipStream_t)hip_stream, err)) return fail(status, err);
    set_ok(status);
    return 0;
}

int gwb_groth16_proofs_decompress_device(const void* d_in, size_t batch, void* d_proofs, void* d_status, void* hip_stream, gw_status_t* status) {
    if (batch && (!d_in || !d_proofs || !d_status)) return fail(status, "gwb_groth16_proofs_decompress_device: NULL argument");
    if (batch > 0x7fffffffull) return fail(status, "gwb_groth16_proofs_decompress_device: batch above 2^31 - 1");
    std::string err;
    if (batch && !enqueue_decompress_proofs((const uint8_t*)d_in, batch, (uint8_t*)d_proofs, (uint32_t*)d_status, (hipStream_t)hip_stream, err))
        return fail(status, err);
    set_ok(status);
    return 0;
}

int gwb_groth16_verify_batch_compressed_device(gwb_g16vk_t* vk, const void* d_cproofs, const void* d_public, size_t n_public, size_t batch,
                                               void* d_status, void* hip_stream, gw_status_t* status) {
    if (!vk || (batch && (!d_cproofs || !d_status || (n_public && !d_public))))
        return fail(status, "gwb_groth16_verify_batch_compressed_device: NULL argument");
    std::string err = verify_args(vk, n_public, batch);
    if (!err.empty()) return fail(status, err);
    if (batch && !enqueue_verify_compressed(vk, (const uint8_t*)d_cproofs, d_public, n_public, batch, (uint32_t*)d_status, (hipStream_t)hip_stream, err))
        return fail(status, err);
    set_ok(status);
    return 0;
}

int gwb_groth16_verify_batch_compressed_host(gwb_g16vk_t* vk, const void* cproofs, const void* pub, size_t n_public, size_t batch, void* status_out,
                                             gw_status_t* status) {
    if (!vk || (batch && (!cproofs || !status_out || (n_public && !pub)))) return fail(status, "gwb_groth16_verify_batch_compressed_host: NULL argument");
    std::string err = verify_args(vk, n_public, batch);
    if (!err.empty()) return fail(status, err);
    if (batch == 0) {
        set_ok(status);
        return 0;
    }
    const size_t pb = batch * GWB_GROTH16_CPROOF_BYTES, sb = batch * n_public * 32;
    Carve c;  // one allocation: the proofs, the public signals, the statuses
    const size_t o_proofs = c.take(pb), o_pub = c.take(sb), o_st = c.take(batch * 4);
    auto run = [&](unsigned char* const* d, hipStream_t s, std::string& err) {
        return enqueue_verify_compressed(vk, d[0] + o_proofs, d[0] + o_pub, n_public, batch, (uint32_t*)(d[0] + o_st), s, err);
    };
    if (!run_staged({c.o}, {{cproofs, pb, 0, o_proofs}, {pub, sb, 0, o_pub}}, {{status_out, batch * 4, 0, o_st}}, "staging the compressed proofs",
                    "running the verifier", run, err))
        return fail(status, err);
    set_ok(status);
    return 0;
}

int gwb_g16vk_load_compressed(const void* bytes, size_t len, gwb_g16vk_t** out, gw_status_t* status) {
    if (!out || (!bytes && len)) return fail(status, "gwb_g16vk_load_compressed: NULL argument");
    *out = nullptr;
    if (len < CKEY_FIXED + 32 || (len - CKEY_FIXED) % 32 != 0)
        return fail(status, "verifying key: " + std::to_string(len) + " bytes (a compressed key has 232 + 32 (nPublic + 1))");
    const uint8_t* b = (const uint8_t*)bytes;
    const uint64_t n_ic = (len - CKEY_FIXED) / 32;
    uint64_t prefix = 0;
    memcpy(&prefix, b + CKEY_FIXED - 8, 8);  // little-endian hosts only, as the rest of the library
    if (prefix != n_ic)
        return fail(status, "verifying key: the length prefix counts " + std::to_string(prefix) + " IC points, the bytes hold " + std::to_string(n_ic));
    if (n_ic - 1 > (1u << 24)) return fail(status, "verifying key: nPublic " + std::to_string(n_ic - 1) + " is above 2^24");
    std::vector<uint8_t> pts;
    try {
        pts.resize(KEY_FIXED + 64 * n_ic);
    } catch (const std::bad_alloc&) {
        return fail(status, "verifying key: out of host memory");
    }
    auto refused = [&](const std::string& what) { return fail(status, "verifying key: " + what + " is not a valid compressed point"); };
    if (g1_decode(b, true, pts.data()) != CODEC_OK) return refused("alpha1");
    const char* names[3] = {"beta2", "gamma2", "delta2"};
    for (size_t k = 0; k < 3; ++k)
        if (g2_decode(b + 32 + 64 * k, true, pts.data() + 64 + 128 * k) != CODEC_OK) return refused(names[k]);
    for (uint64_t i = 0; i < n_ic; ++i)
        if (g1_decode(b + CKEY_FIXED + 32 * i, true, pts.data() + KEY_FIXED + 64 * i) != CODEC_OK) return refused("IC[" + std::to_string(i) + "]");
    return gwb_g16vk_load(pts.data(), pts.size(), (uint32_t)(n_ic - 1), out, status);
}

int gwb_g16vk_compressed(const gwb_g16vk_t* vk, void* out, size_t len) {
    gwb_g16vk_info_t info{};
    if (!vk || !out || gwb_g16vk_info(vk, &info) != 0 || len != GWB_G16VK_COMPRESSED_BYTES(info.n_public)) return 1;
    const uint64_t n_ic = (uint64_t)info.n_public + 1;
    std::vector<uint8_t> pts(KEY_FIXED + 64 * n_ic);
    if (gwb_g16vk_points(vk, pts.data(), pts.size()) != 0) return 1;
    uint8_t* o = (uint8_t*)out;
    g1_encode(pts.data(), true, o);
    for (size_t k = 0; k < 3; ++k) g2_encode(pts.data() + 64 + 128 * k, true, o + 32 + 64 * k);
    memcpy(o + CKEY_FIXED - 8, &n_ic, 8);
    for (uint64_t i = 0; i < n_ic; ++i) g1_encode(pts.data() + KEY_FIXED + 64 * i, true, o + CKEY_FIXED + 32 * i);
    return 0;
}

}  // extern "C"
