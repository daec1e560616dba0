// Groth16 phase-2 contributions on gfx950 (include/graph_witness_groth16_contribute.h has the definitions): the contribution
// itself, the check of a key's records, the check of one step between two keys, the check of a key against its circuit and its
// powers-of-tau file, and the powers check and the Lagrange check of such a file (include/graph_witness_groth16_ptau.h).  Section 10, BLAKE2b, the
// transcript and the challenge point are contributions.cc's (contribute_internal.hpp); the pairing is verify.hip's and the
// conversion to affine bytes setup.hip's, both through their enqueue functions.
//
// Contribute.  The few single points (g1_s, g1_sx, g2_spx, delta1, delta2) are multiplied on the host.  Sections 8 and 9 are one
// list of stored G1 points that goes through the device in pieces of CWC_CONTRIBUTE_CHUNK points: scale_points_kernel decodes
// a point and multiplies it by 1 / delta (fq_gfx950.hpp's xyzz_mul_short; the scalar is read through one uniform address, so
// a wave takes the additions of the scalar's one bits together), then the shared-inversion kernel writes the stored bytes, zero
// bytes for infinity.  1 / delta lives in a device buffer that is zeroed before it is released.
//
// Step check.  R = sum rho_i P_i over a section of the previous key and R' over the same section of the next key, rho_i of 128
// bits, the same for both: lincomb_kernel takes one point per thread (blockIdx.y picks the list), multiplies it by its rho
// (four words of double-and-add) and the workgroup adds its products through LDS, halving the active threads each round;
// lincomb_sum_kernel, one workgroup per list, adds the per-group sums to the running sum of the list.  The bucket method of
// msm.hip was not reused: it is built around the prover's resident bases and 254-bit scalars, and this sum is a small part
// of a step check next to its pairings.
//
// Key check.  The key of the circuit and the file with delta = 1 is remade (gwb_groth16_setup_ptau) and takes the place of the
// previous key of a step whose secret is the whole delta: the same functions compare the sections, check the records and the
// delta points and form R and R', and one run_checks carries all pairings.
//
// Powers check.  Sums over the file's own lists with one rho: tauG1 against itself one point on (U, V, and V_n as V's state
// after the first n points), alphaTauG1 and betaTauG1 as the two lists of one launch, and tauG2 through the G2 instance of the
// two kernels.  Both kernels are templates over the group.  A G1 workgroup has 256 threads.  A G2 workgroup is one wave of
// 64: an Xyzz<G2> is 256 bytes (256 of them would be 64 KB of LDS), and the G2 double-and-add keeps the multiplicand, the
// accumulator and an addition's temporaries, which needs the unified register file of a wave that has its SIMD to itself.
// The lengths of the sums are arguments (powers_rules): the prefixes of one setup here, every point of the file for the
// ceremony's verification (ceremony.hip, gwb_ptau_verify), which shares the sums, the equations and the batched pairings
// through contribute_internal.hpp.
//
// Lagrange check (gwb_ptau_check_lagrange; the header has the equation).  Per section and set of levels, the left side is
// lincomb_kernel over the Lagrange points with the 128-bit rho of their slots, as above.  The right side multiplies the
// monomial points by c, the same transform applied to rho, which has the full width of r: lincomb_kernel takes the scalar's
// words as a template parameter, 4 or 8 (xyzz_mul_short starts from the top nonzero word either way; the four-word
// instantiations are the kernels of the checks above, unchanged).  c is made on the device in the section's all-level layout:
// rho_levels_kernel (widened to eight words, bit-reversed per level; the values stay canonical and only the twiddles and
// 1 / 2^m are in Montgomery form, so nothing is converted), fr_levels_stage_kernel once per stage for all levels (the thread
// layout of setup_ptau.hip's idft_levels_stage_kernel), fold_levels_kernel (the factor 1 / 2^m and the sum over the
// levels, canonical).  qap.hip's passes were not used: they transform rows of one length on a handle's tables.  The two sums
// are converted to affine bytes and compared on the host.  rho is uploaded once per call and neither it nor c comes back.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage for gfx950; every kernel: 0 bytes of scratch; VGPRs + AGPRs, waves / SIMD):
//   scale_points_kernel 156, 3      lincomb_kernel<G1, 4> 164, 3 (32 KB LDS)      lincomb_sum_kernel<G1> 119, 4 (32 KB LDS)      put_scalar_kernel 10, 8
//   lincomb_kernel<G2, 4> 256 + 79, 1 (16 KB LDS)      lincomb_sum_kernel<G2> 256 + 12, 1 (16 KB LDS)
//   lincomb_kernel<G1, 8> 166, 3 (32 KB LDS)           lincomb_kernel<G2, 8> 256 + 80, 1 (16 KB LDS)
//   rho_levels_kernel 11, 8      fr_powers_kernel 35, 8      fr_levels_stage_kernel 42, 8      fold_levels_kernel 57, 8
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <chrono>
#include <initializer_list>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/graph_witness_groth16_beacon.h"
#include "../../include/graph_witness_groth16_contribute.h"
#include "../../include/graph_witness_groth16_ptau.h"
#include "../../include/graph_witness_groth16_setup.h"
#include "../../include/graph_witness_groth16_verify.h"
#include "beacon.hpp"
#include "binfile.hpp"
#include "bn254_points_gfx950.hpp"
#include "contribute_internal.hpp"
#include "groth16_internal.hpp"
#include "ptau_internal.hpp"
#include "setup_internal.hpp"

using namespace cwc_r1cs;
using namespace cwc_g16;
using namespace cwc_contrib;
using cwc::Fr;
using cwc_setup::enqueue_affine_g1;

namespace {

constexpr uint32_t THREADS = 256;
constexpr size_t RHO_BYTES = 16;

// out[i] = k in[i] for the stored points in[0 .. n) (Montgomery, or canonical), XYZZ
__global__ __launch_bounds__(THREADS) void scale_points_kernel(const uint8_t* __restrict__ in, uint32_t n, uint32_t canonical, const Fr* __restrict__ k,
                                                               Xyzz<G1>* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    A1 a;
    get_coords<G1>(in + (size_t)i * G1_BYTES, canonical != 0, a.x, a.y);
    out[i] = xyzz_mul_short(from_affine(a), *k);
}

// *out = v (a scalar for scale_points_kernel without a copy from host memory)
__global__ __launch_bounds__(64) void put_scalar_kernel(Fr* __restrict__ out, Fr v) {
    if (threadIdx.x == 0) *out = v;
}

// threads of a workgroup of the linear-combination kernels, and the stored bytes of a point, per group (the header has the why)
template <class T>
constexpr uint32_t LC_THREADS = THREADS;
template <>
constexpr uint32_t LC_THREADS<G2> = 64;
template <class T>
constexpr size_t POINT_BYTES = G1_BYTES;
template <>
constexpr size_t POINT_BYTES<G2> = G2_BYTES;

// the sum of sh[0 .. LC_THREADS<T>) into sh[0]
template <class T>
__device__ __forceinline__ void block_sum(Xyzz<T>* sh) {
    __syncthreads();
    for (uint32_t stride = LC_THREADS<T> / 2; stride > 0; stride >>= 1) {
        if (threadIdx.x < stride) sh[threadIdx.x] = xyzz_add(sh[threadIdx.x], sh[threadIdx.x + stride]);
        __syncthreads();
    }
}

// part[blockIdx.y gridDim.x + blockIdx.x] = sum over the workgroup's i of rho[i] P_i, P = in0 or (blockIdx.y = 1) in1; rho[i] has
// WORDS words: 4 (the 128-bit rho of the step, key and powers checks) or 8 (canonical scalars below r: the Lagrange check's c)
template <class T, uint32_t WORDS>
__global__ __launch_bounds__(LC_THREADS<T>) void lincomb_kernel(const uint8_t* __restrict__ in0, const uint8_t* __restrict__ in1, uint32_t n,
                                                                uint32_t canonical, const uint32_t* __restrict__ rho, Xyzz<T>* __restrict__ part) {
    static_assert(WORDS == 4 || WORDS == 8, "a scalar of 4 or 8 words");
    __shared__ Xyzz<T> sh[LC_THREADS<T>];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Xyzz<T> acc = xyzz_inf<T>();
    if (i < n) {
        const uint8_t* in = blockIdx.y ? in1 : in0;
        Affine<T> a;
        get_coords<T>(in + (size_t)i * POINT_BYTES<T>, canonical != 0, a.x, a.y);
        const uint32_t* r = rho + WORDS * (size_t)i;
        if constexpr (WORDS == 4)
            acc = xyzz_mul_short(from_affine(a), Fr{{r[0], r[1], r[2], r[3], 0, 0, 0, 0}});
        else
            acc = xyzz_mul_short(from_affine(a), Fr{{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]}});
    }
    sh[threadIdx.x] = acc;
    block_sum<T>(sh);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sh[0];
}

// acc[blockIdx.x] += sum of part[blockIdx.x n_part .. + n_part)
template <class T>
__global__ __launch_bounds__(LC_THREADS<T>) void lincomb_sum_kernel(const Xyzz<T>* __restrict__ part, uint32_t n_part, Xyzz<T>* __restrict__ acc) {
    __shared__ Xyzz<T> sh[LC_THREADS<T>];
    Xyzz<T> s = xyzz_inf<T>();
    for (uint32_t j = threadIdx.x; j < n_part; j += LC_THREADS<T>) s = xyzz_add(s, part[(size_t)blockIdx.x * n_part + j]);
    sh[threadIdx.x] = s;
    block_sum<T>(sh);
    if (threadIdx.x == 0) acc[blockIdx.x] = xyzz_add(acc[blockIdx.x], sh[0]);
}

// The Lagrange check's scalars (the header's "Lagrange check"): the transform of setup_ptau.hip's idft_levels_stage_kernel on
// field elements in the same all-level layout, level m in the slots [2^m - 1, 2^(m+1) - 1).  N log N field products next to
// the N point multiplications they feed: plain radix 2 in global memory.

// x[slot of level m, position bitrev_m(k)] = rho_i, for the slots i = 2^m - 1 + k in [lo, hi).  The values stay canonical through
// the transform: the product of a canonical value with a twiddle in Montgomery form is their canonical product.
__global__ __launch_bounds__(THREADS) void rho_levels_kernel(const uint32_t* __restrict__ rho, uint32_t lo, uint32_t hi, Fr* __restrict__ x) {
    const uint32_t i = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hi) return;
    const uint32_t m = 31u - (uint32_t)__builtin_clz(i + 1u), first = (1u << m) - 1u, k = i - first;
    const uint32_t* r = rho + 4 * (size_t)i;
    x[first + (m ? __brev(k) >> (32 - m) : 0u)] = Fr{{r[0], r[1], r[2], r[3], 0, 0, 0, 0}};
}

// out[k] = base^k in Montgomery form for k < count (bp.v[b] = base^(2^b))
__global__ __launch_bounds__(THREADS) void fr_powers_kernel(Fr* __restrict__ out, uint32_t count, Pows bp) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    Fr x = cwc::fr_one();
    for (uint32_t b = 0; b <= MAX_DOMAIN_POWER; ++b)
        if ((k >> b) & 1u) x = cwc::fr_mul(x, bp.v[b]);
    out[k] = x;
}

// stage s of the levels m in [max(m_lo, s + 1), top]; tw[k << tw_shift] = w_(2^(s+1))^(-k), Montgomery form; 2^top threads
__global__ __launch_bounds__(THREADS) void fr_levels_stage_kernel(Fr* __restrict__ x, uint32_t top, uint32_t s, uint32_t m_lo, uint32_t tw_shift,
                                                                  const Fr* __restrict__ tw) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    cwc_ptau::LevelButterfly b;
    if ((v >> top) != 0 || !cwc_ptau::level_butterfly(v, top, s, b) || b.m < m_lo) return;
    Fr* lo = x + (((size_t)1 << b.m) - 1) + ((size_t)b.grp << (s + 1)) + b.k;
    const Fr a = lo[0], c = cwc::fr_mul(lo[(size_t)1 << s], tw[(size_t)b.k << tw_shift]);
    lo[0] = cwc::fr_add(a, c);
    lo[(size_t)1 << s] = cwc::fr_sub(a, c);
}

struct InvPowersOfTwo {
    Fr v[cwc_ptau::MAX_POWER + 2];  // 1 / 2^m, Montgomery form
};

// c[i] = sum over the levels m in [m_lo, m_hi] with 2^m > i of x[2^m - 1 + i] / 2^m, canonical, for i < 2^m_hi
__global__ __launch_bounds__(THREADS) void fold_levels_kernel(const Fr* __restrict__ x, uint32_t m_lo, uint32_t m_hi, InvPowersOfTwo inv, Fr* __restrict__ c) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if ((i >> m_hi) != 0) return;
    Fr acc = cwc::fr_zero();
    for (uint32_t m = m_lo; m <= m_hi; ++m)
        if ((i >> m) == 0) acc = cwc::fr_add(acc, cwc::fr_mul(x[(((size_t)1 << m) - 1) + i], inv.v[m]));
    c[i] = acc;
}

// ---- host -----------------------------------------------------------------------------------------------------------------

int fail2(gw_status_t* status, const std::string& msg) {  // a failure that is not a verdict about the key
    set_status(status, msg);
    return 2;
}

uint64_t chunk_points() { return piece_points("CWC_CONTRIBUTE_CHUNK"); }

struct ZkeyFree {
    void operator()(gwb_zkey_t* z) const { gwb_zkey_free(z); }
};
using ZkeyPtr = std::unique_ptr<gwb_zkey_t, ZkeyFree>;

// A key as the three functions read it: checked by the loader, its section table and its section 10.
struct Key {
    ZkeyPtr z;
    BinSection secs[11];
    Section10 s10;
};

bool read_key(const void* data, size_t len, Key& k, std::string& err) {
    gw_status_t st{};
    gwb_zkey_t* z = nullptr;
    if (gwb_zkey_load(data, len, &z, &st) != 0) {
        err = st.error_msg ? st.error_msg : "zkey: not loaded";
        free(st.error_msg);
        return false;
    }
    k.z.reset(z);
    if (!binfile_sections((const uint8_t*)data, len, "zkey", 0x7feu, k.secs, err)) return false;
    if (!k.secs[10].p) {
        err = "zkey: section 10 is missing";
        return false;
    }
    return parse_section10(k.secs[10].p, k.secs[10].size, k.s10, err);
}

// H(the bodies of sections 1 to 9 in id order)
void sections_hash(const BinSection* secs, uint8_t out[HASH_BYTES]) {
    Blake2b h;
    for (uint32_t id = 1; id <= 9; ++id) h.update(secs[id].p, secs[id].size);
    h.final(out);
}

bool is_zero_bytes(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (p[i]) return false;
    return true;
}

struct Secrets {
    Fr delta, delta_inv, s;  // canonical
    ~Secrets() { explicit_bzero(this, sizeof *this); }
};

bool draw_nonzero(Fr& x, std::string& err) {
    do {
        if (!draw_fr(x, err)) return false;
    } while (cwc::u256_is_zero(x));
    return true;
}

PhaseTimes<3> g_phases;

// out = k in for the n stored points at `in`, in pieces; d_k is the device address of the canonical scalar
bool scale_list(const uint8_t* in, uint64_t n, const Fr* d_k, SetupDevice<4>& D, uint64_t chunk, uint8_t* out, std::string& err) {
    uint8_t* W = D.work.as<uint8_t>();
    Carve cw;
    const size_t o_in = cw.take(chunk * G1_BYTES), o_x = cw.take(chunk * sizeof(Xyzz<G1>)), o_out = cw.take(chunk * G1_BYTES);
    float total[3] = {0, 0, 0};
    bool timed = true;
    for (uint64_t at = 0; at < n; at += chunk) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - at);
        D.ev.record(0, D.s);
        hipError_t e = hipMemcpyAsync(W + o_in, in + at * G1_BYTES, (size_t)m * G1_BYTES, hipMemcpyHostToDevice, D.s);
        if (e != hipSuccess) {
            err = hip_err("uploading the points of sections 8 and 9", e);
            return false;
        }
        D.ev.record(1, D.s);
        hipLaunchKernelGGL(scale_points_kernel, dim3(blocks_for(m, THREADS)), dim3(THREADS), 0, D.s, (const uint8_t*)(W + o_in), m, 0u, d_k, (Xyzz<G1>*)(W + o_x));
        D.ev.record(2, D.s);
        enqueue_affine_g1(W + o_x, m, W + o_out, false, D.s);
        D.ev.record(3, D.s);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out + at * G1_BYTES, W + o_out, (size_t)m * G1_BYTES, hipMemcpyDeviceToHost, D.s);
        if (e == hipSuccess) e = hipStreamSynchronize(D.s);
        if (e != hipSuccess) {
            err = hip_err("scaling the points of sections 8 and 9", e);
            return false;
        }
        float t[3];
        if (D.ev.elapsed(t) == hipSuccess)
            for (int i = 0; i < 3; ++i) total[i] += t[i];
        else
            timed = false;
    }
    g_phases.store(total, timed);
    return true;
}

void put32(std::vector<uint8_t>& v, uint32_t x) { v.insert(v.end(), (const uint8_t*)&x, (const uint8_t*)&x + 4); }
void put_section(std::vector<uint8_t>& v, uint32_t id, const uint8_t* p, size_t n) {
    const uint64_t size = n;
    put32(v, id);
    v.insert(v.end(), (const uint8_t*)&size, (const uint8_t*)&size + 8);
    v.insert(v.end(), p, p + n);
}

constexpr size_t HDR_DELTA1 = 84 + 2 * G1_BYTES + 2 * G2_BYTES, HDR_DELTA2 = HDR_DELTA1 + G1_BYTES;  // in section 2

// The one path of a contribution and of a beacon: the secret sec.delta and the nonce sec.s, both in [1, r), are applied to the
// parsed key, and the record of the given type with the given parameters is appended.
int apply(const Key& key, size_t len, Secrets& sec, uint32_t type, const std::vector<uint8_t>& params, const std::string& nm, void** out, size_t* out_len,
          uint8_t* hash64, gw_status_t* status) {
    std::string err;
    sec.delta_inv = cwc::fr_from_mont(cwc::fr_inv_fermat(cwc::fr_to_mont(sec.delta)));
    const gwb_zkey& z = *key.z;
    Section10 s10 = key.s10;
    if (s10.blank()) sections_hash(key.secs, s10.cs_hash);
    Record rec;
    uint8_t gen1[G1_BYTES], g2_sp[G2_BYTES];
    put_stored(gen1, g1_generator());
    g1_mul_stored(gen1, sec.s, rec.g1_s);
    g1_mul_stored(rec.g1_s, sec.delta, rec.g1_sx);
    transcript_of(s10, s10.recs.size(), rec.g1_s, rec.g1_sx, rec.transcript);
    put_stored(g2_sp, hash_to_g2(rec.transcript));
    g2_mul_stored(g2_sp, sec.delta, rec.g2_spx);
    uint8_t delta2[G2_BYTES];
    g1_mul_stored(z.delta1, sec.delta, rec.delta_after);
    g2_mul_stored(z.delta2, sec.delta, delta2);
    rec.type = type;
    rec.params = params;
    rec.name = nm;
    record_hash(rec, hash64);
    s10.recs.push_back(rec);

    // sections 8 and 9 as one list
    const uint64_t n_c = z.c.size() / G1_BYTES, n_h = z.h.size() / G1_BYTES, n = n_c + n_h;
    std::vector<uint8_t> pts(n * G1_BYTES), scaled(n * G1_BYTES);
    memcpy(pts.data(), z.c.data(), z.c.size());
    memcpy(pts.data() + z.c.size(), z.h.data(), z.h.size());
    {
        SetupDevice<4> D;
        const uint64_t chunk = std::max<uint64_t>(1, std::min(chunk_points(), n));
        Carve cw;
        cw.take(chunk * G1_BYTES);
        cw.take(chunk * sizeof(Xyzz<G1>));
        cw.take(chunk * G1_BYTES);
        hipError_t e = D.open(256, cw.o);
        if (e != hipSuccess) return fail(status, hip_err("allocating the contribution's workspace", e));
        e = hipMemcpyAsync(D.secret.as(), &sec.delta_inv, sizeof(Fr), hipMemcpyHostToDevice, D.s);
        if (e == hipSuccess) e = hipStreamSynchronize(D.s);  // the copy has left the host value
        if (e != hipSuccess) return fail(status, hip_err("uploading the contribution's scalar", e));
        if (!scale_list(pts.data(), n, D.secret.as<const Fr>(), D, chunk, scaled.data(), err)) return fail(status, err);
        e = hipMemsetAsync(D.secret.as(), 0, D.secret_bytes, D.s);
        if (e == hipSuccess) e = hipStreamSynchronize(D.s);
        if (e != hipSuccess) return fail(status, hip_err("clearing the contribution's scalar", e));
    }

    std::vector<uint8_t> hdr(key.secs[2].p, key.secs[2].p + key.secs[2].size), sec10, file;
    memcpy(hdr.data() + HDR_DELTA1, rec.delta_after, G1_BYTES);
    memcpy(hdr.data() + HDR_DELTA2, delta2, G2_BYTES);
    write_section10(s10, sec10);
    file.reserve(len + sec10.size() + 64);
    file.insert(file.end(), {'z', 'k', 'e', 'y'});
    put32(file, 1);
    put32(file, 10);
    for (uint32_t id = 1; id <= 10; ++id) {
        if (id == 2)
            put_section(file, id, hdr.data(), hdr.size());
        else if (id == 8)
            put_section(file, id, scaled.data(), n_c * G1_BYTES);
        else if (id == 9)
            put_section(file, id, scaled.data() + n_c * G1_BYTES, n_h * G1_BYTES);
        else if (id == 10)
            put_section(file, id, sec10.data(), sec10.size());
        else
            put_section(file, id, key.secs[id].p, key.secs[id].size);
    }
    void* buf = malloc(file.size());
    if (!buf) return fail(status, "groth16 contribute: out of host memory");
    memcpy(buf, file.data(), file.size());
    *out = buf;
    *out_len = file.size();
    set_ok(status);
    return 0;
}

int contribute(const uint8_t* zkey, size_t len, const char* name, const uint8_t* delta, void** out, size_t* out_len, uint8_t* hash64,
               gw_status_t* status) {
    std::string err;
    Key key;
    if (!read_key(zkey, len, key, err)) return fail(status, err);
    const std::string nm = name ? name : "";
    if (nm.size() > GWB_CONTRIBUTION_NAME_MAX)
        return fail(status, "groth16 contribute: the name has " + std::to_string(nm.size()) + " bytes, 255 at the most");
    Secrets sec;
    if (delta) {
        memcpy(sec.delta.v, delta, 32);
        if (cwc::u256_is_zero(sec.delta) || !cwc::u256_lt(sec.delta, cwc::fr_p())) return fail(status, "groth16 contribute: delta is not in [1, r)");
    } else if (!draw_nonzero(sec.delta, err)) {
        return fail(status, err);
    }
    if (!draw_nonzero(sec.s, err)) return fail(status, err);
    return apply(key, len, sec, 0, name_params(nm), nm, out, out_len, hash64, status);
}

// A beacon is the contribution whose secret and nonce its parameters give (beacon.hpp); they are public, so that the zeroing of
// `Secrets` protects nothing here.  Every failure returns 2: none is a verdict.
int beacon(const uint8_t* zkey, size_t len, const char* name, const uint8_t* hash, size_t hash_len, uint32_t exp, void** out, size_t* out_len,
           uint8_t* hash64, gw_status_t* status) {
    const std::string nm = name ? name : "";
    const std::string fault = cwc_beacon::argument_fault(nm.size(), hash_len, exp, cwc_beacon::limit());
    if (!fault.empty()) return fail2(status, fault);
    std::string err;
    Key key;
    if (!read_key(zkey, len, key, err)) return fail2(status, err);
    Fr derived[cwc_beacon::PHASE2_SCALARS];
    cwc_beacon::scalars(2, hash, hash_len, exp, derived);
    Secrets sec;
    sec.delta = derived[0];
    sec.s = derived[1];
    return apply(key, len, sec, 1, cwc_beacon::write_params(nm, exp, hash, hash_len), nm, out, out_len, hash64, status) == 0 ? 0 : 2;
}

// ---- verification -----------------------------------------------------------------------------------------------------------

// The host rules of record k of s (its transcript, no infinity, g2_spx in the subgroup); "" or what fails.  The record's two
// pairing rules go to `checks`; g2_sp (stored) gets the record's challenge point and has to outlive the checks.
std::string record_rules(const Section10& s, size_t k, const uint8_t* delta_prev, uint8_t* g2_sp, std::vector<PairCheck>& checks) {
    const Record& r = s.recs[k];
    const std::string who = "zkey: contribution " + std::to_string(k + 1) + ": ";
    uint8_t t[HASH_BYTES];
    transcript_of(s, k, r.g1_s, r.g1_sx, t);
    if (memcmp(t, r.transcript, HASH_BYTES) != 0) return who + "the transcript is not that of the csHash, the records before it and g1_s, g1_sx";
    const struct {
        const char* name;
        const uint8_t* at;
        size_t bytes;
    } pts[4] = {{"deltaAfter", r.delta_after, G1_BYTES}, {"g1_s", r.g1_s, G1_BYTES}, {"g1_sx", r.g1_sx, G1_BYTES}, {"g2_spx", r.g2_spx, G2_BYTES}};
    for (const auto& p : pts)
        if (is_zero_bytes(p.at, p.bytes)) return who + p.name + " is the point at infinity";
    if (!g2_stored_in_subgroup(r.g2_spx)) return who + "g2_spx is not in the order-r subgroup of G2";
    put_stored(g2_sp, hash_to_g2(t));
    checks.push_back({r.g1_s, r.g2_spx, r.g1_sx, g2_sp, who + "g1_sx is not g1_s times the secret that g2_spx proves"});
    checks.push_back({delta_prev, r.g2_spx, r.delta_after, g2_sp, who + "deltaAfter is not deltaPrev times the proven secret"});
    if (r.type == 1) {  // the beacon rule: g1_s and g1_sx are those of the derived secret and nonce; the pairings above fix the rest
        const cwc_beacon::Form f = cwc_beacon::form_of(r.params, cwc_beacon::MAX_EXP);  // form and limit were checked before the device
        if (f.rc != 0) return who + f.msg;
        Fr derived[cwc_beacon::PHASE2_SCALARS];
        cwc_beacon::scalars(2, f.items.hash, f.items.hash_len, f.items.exp, derived);
        uint8_t gen1[G1_BYTES], g1_s[G1_BYTES], g1_sx[G1_BYTES];
        put_stored(gen1, g1_generator());
        g1_mul_stored(gen1, derived[1], g1_s);
        g1_mul_stored(g1_s, derived[0], g1_sx);
        if (memcmp(g1_s, r.g1_s, G1_BYTES) != 0 || memcmp(g1_sx, r.g1_sx, G1_BYTES) != 0)
            return who + "the key is not the one its beaconHash and numIterationsExp give";
    }
    return "";
}

// The rules about the header's delta points after the last record (`last`: its deltaAfter, or nullptr without records): delta1
// continues the chain, then delta2 belongs to delta1.  The key check asks the second alone when it passes over the records.
std::string delta1_rule(const gwb_zkey& z, const uint8_t* last, const uint8_t* gen1) {
    if (!last && memcmp(z.delta1, gen1, G1_BYTES) != 0) return "zkey: delta is not the generator and no contribution accounts for it";
    if (last && memcmp(z.delta1, last, G1_BYTES) != 0) return "zkey: delta1 is not the deltaAfter of the last contribution";
    return "";
}
std::string delta2_rules(const gwb_zkey& z, const uint8_t* gen1, const uint8_t* gen2, std::vector<PairCheck>& checks) {
    if (is_zero_bytes(z.delta2, G2_BYTES)) return "zkey: delta2 is the point at infinity";
    if (!g2_stored_in_subgroup(z.delta2)) return "zkey: delta2 is not in the order-r subgroup of G2";
    checks.push_back({z.delta1, gen2, gen1, z.delta2, "zkey: delta2 is not the G2 generator times delta1's scalar"});
    return "";
}
std::string delta_rules(const gwb_zkey& z, const uint8_t* last, const uint8_t* gen1, const uint8_t* gen2, std::vector<PairCheck>& checks) {
    const std::string v = delta1_rule(z, last, gen1);
    return v.empty() ? delta2_rules(z, gen1, gen2, checks) : v;
}

// e(a1, a2) = e(b1, b2) where a side with a point at infinity is 1: one such side alone is the failure `msg`, two pass without
// a pairing, none goes to `checks`.
std::string pair_rule(const uint8_t* a1, const uint8_t* a2, const uint8_t* b1, const uint8_t* b2, const std::string& msg, std::vector<PairCheck>& checks) {
    const bool inf_a = is_zero_bytes(a1, G1_BYTES) || is_zero_bytes(a2, G2_BYTES), inf_b = is_zero_bytes(b1, G1_BYTES) || is_zero_bytes(b2, G2_BYTES);
    if (inf_a != inf_b) return msg;
    if (!inf_a) checks.push_back({a1, a2, b1, b2, msg});
    return "";
}

// Runs the pairings of `checks` in one batched launch; verdict = the message of the first check that fails, "" if none does.
bool run_checks(const std::vector<PairCheck>& checks, std::string& verdict, std::string& err) {
    verdict.clear();
    const size_t n = 2 * checks.size();
    if (n == 0) return true;
    std::vector<uint8_t> g1(n * G1_BYTES), g2(n * G2_BYTES), gt(n * GWB_GT_BYTES);
    for (size_t i = 0; i < checks.size(); ++i) {
        canonical_g1(checks[i].a1, g1.data() + 2 * i * G1_BYTES);
        canonical_g2(checks[i].a2, g2.data() + 2 * i * G2_BYTES);
        canonical_g1(checks[i].b1, g1.data() + (2 * i + 1) * G1_BYTES);
        canonical_g2(checks[i].b2, g2.data() + (2 * i + 1) * G2_BYTES);
    }
    auto run = [&](unsigned char** d, hipStream_t s, std::string& e) {
        gw_status_t st{};
        if (gwb_bn254_pairing_batch_device(d[0], d[1], n, d[2], s, &st) != 0) {
            e = st.error_msg ? st.error_msg : "pairing failed";
            free(st.error_msg);
            return false;
        }
        return true;
    };
    if (!run_staged({g1.size(), g2.size(), gt.size()}, {{g1.data(), g1.size(), 0, 0}, {g2.data(), g2.size(), 1, 0}}, {{gt.data(), gt.size(), 2, 0}},
                    "staging the pairings of the contribution check", "running the pairings of the contribution check", run, err))
        return false;
    for (size_t i = 0; i < checks.size(); ++i)
        if (memcmp(gt.data() + 2 * i * GWB_GT_BYTES, gt.data() + (2 * i + 1) * GWB_GT_BYTES, GWB_GT_BYTES) != 0) {
            verdict = checks[i].msg;
            return true;
        }
    return true;
}

struct Generators {
    uint8_t g1[G1_BYTES], g2[G2_BYTES];
    Generators() {
        put_stored(g1, g1_generator());
        put_stored(g2, g2_generator());
    }
};

int verify_contributions(const uint8_t* zkey, size_t len, uint8_t* hashes_out, size_t* n_io, gw_status_t* status) {
    std::string err;
    Key key;
    if (!read_key(zkey, len, key, err)) return fail2(status, err);
    const Section10& s = key.s10;
    if (const int rc = cwc_beacon::forms_of(s.recs, 0, "zkey", err)) return rc == 1 ? fail(status, err) : fail2(status, err);
    const size_t n = s.recs.size();
    const Generators gen;
    std::vector<PairCheck> checks;
    std::vector<uint8_t> sp(std::max<size_t>(n, 1) * G2_BYTES);
    std::string host_verdict;  // the first host rule that fails; the pairing rules of the records before it come first
    for (size_t k = 0; k < n && host_verdict.empty(); ++k)
        host_verdict = record_rules(s, k, k ? s.recs[k - 1].delta_after : gen.g1, sp.data() + k * G2_BYTES, checks);
    if (host_verdict.empty()) host_verdict = delta_rules(*key.z, n ? s.recs[n - 1].delta_after : nullptr, gen.g1, gen.g2, checks);
    std::string verdict;
    if (!run_checks(checks, verdict, err)) return fail2(status, err);
    if (verdict.empty()) verdict = host_verdict;
    if (!verdict.empty()) return fail(status, verdict);
    const size_t room = *n_io;
    *n_io = n;
    for (size_t k = 0; k < n && k < room && hashes_out; ++k) record_hash(s.recs[k], hashes_out + k * HASH_BYTES);
    set_ok(status);
    return 0;
}

// rho_i for i in [first, first + count): four per digest H(seed || u64le(j)), j = i / 4
void fill_rho(const uint8_t seed[32], uint64_t first, uint64_t count, uint8_t* out) {
    uint8_t msg[40], d[HASH_BYTES];
    memcpy(msg, seed, 32);
    uint64_t have = ~0ull;
    for (uint64_t i = first; i < first + count; ++i) {
        const uint64_t j = i / 4;
        if (j != have) {
            memcpy(msg + 32, &j, 8);
            blake2b512(msg, sizeof msg, d);
            have = j;
        }
        memcpy(out + (i - first) * RHO_BYTES, d + RHO_BYTES * (i % 4), RHO_BYTES);
    }
}

// d_acc[0] += sum rho_i P_i, d_acc[1] += sum rho_i P'_i over the m points of one piece (device addresses), the per-group sums in
// d_part (lists blocks_for(m, LC_THREADS<T>) points); rho_i of WORDS words
template <class T, uint32_t WORDS = 4>
void enqueue_lincomb(const uint8_t* d_p0, const uint8_t* d_p1, uint32_t lists, uint32_t m, bool canonical, const uint8_t* d_rho, Xyzz<T>* d_part,
                     Xyzz<T>* d_acc, hipStream_t s) {
    const uint32_t blocks = blocks_for(m, LC_THREADS<T>);
    hipLaunchKernelGGL((lincomb_kernel<T, WORDS>), dim3(blocks, lists), dim3(LC_THREADS<T>), 0, s, d_p0, d_p1, m, canonical ? 1u : 0u, (const uint32_t*)d_rho, d_part);
    hipLaunchKernelGGL(lincomb_sum_kernel<T>, dim3(lists), dim3(LC_THREADS<T>), 0, s, (const Xyzz<T>*)d_part, blocks, d_acc);
}

// XYZZ points of either group -> affine bytes (setup.hip's shared inversions)
template <class T>
void enqueue_affine(const void* d_xyzz, uint32_t n, uint8_t* d_out, bool canonical, hipStream_t s) {
    if constexpr (std::is_same<T, G1>::value)
        enqueue_affine_g1(d_xyzz, n, d_out, canonical, s);
    else
        cwc_setup::enqueue_affine_g2(d_xyzz, n, d_out, canonical, s);
}

// The four sums of a step check, stored form in out[4][64]: R and R' of section 8, then of section 9.
bool step_sums(const gwb_zkey& prev, const gwb_zkey& next, const uint8_t seed[32], uint8_t* out, std::string& err) {
    const uint64_t n_c = prev.c.size() / G1_BYTES, n_h = prev.h.size() / G1_BYTES;
    const uint64_t chunk = std::max<uint64_t>(1, std::min(chunk_points(), std::max(n_c, n_h)));
    const uint32_t max_blocks = blocks_for(chunk, THREADS);
    Stream s;
    DeviceBuf work;
    Carve cw;
    const size_t o_p0 = cw.take(chunk * G1_BYTES), o_p1 = cw.take(chunk * G1_BYTES), o_rho = cw.take(chunk * RHO_BYTES),
                 o_part = cw.take(2ull * max_blocks * sizeof(Xyzz<G1>)), o_acc = cw.take(4 * sizeof(Xyzz<G1>)), o_out = cw.take(4 * G1_BYTES);
    hipError_t e = s.create();
    if (e == hipSuccess) e = work.alloc(cw.o);
    if (e == hipSuccess) e = hipMemsetAsync(work.as<uint8_t>() + o_acc, 0, 4 * sizeof(Xyzz<G1>), s);
    if (e != hipSuccess) {
        err = hip_err("allocating the step check's workspace", e);
        return false;
    }
    uint8_t* W = work.as<uint8_t>();
    std::vector<uint8_t> rho(chunk * RHO_BYTES);
    for (int sec = 0; sec < 2; ++sec) {
        const uint8_t *p0 = sec ? prev.h.data() : prev.c.data(), *p1 = sec ? next.h.data() : next.c.data();
        const uint64_t n = sec ? n_h : n_c, base = sec ? n_c : 0;
        for (uint64_t at = 0; at < n; at += chunk) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - at);
            fill_rho(seed, base + at, m, rho.data());
            e = hipMemcpyAsync(W + o_p0, p0 + at * G1_BYTES, (size_t)m * G1_BYTES, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(W + o_p1, p1 + at * G1_BYTES, (size_t)m * G1_BYTES, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(W + o_rho, rho.data(), (size_t)m * RHO_BYTES, hipMemcpyHostToDevice, s);
            if (e != hipSuccess) {
                err = hip_err("uploading the points of a step check", e);
                return false;
            }
            enqueue_lincomb(W + o_p0, W + o_p1, 2, m, false, W + o_rho, (Xyzz<G1>*)(W + o_part), (Xyzz<G1>*)(W + o_acc) + 2 * sec, s);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(s);  // rho is refilled for the next piece
            if (e != hipSuccess) {
                err = hip_err("running the linear combinations of a step check", e);
                return false;
            }
        }
    }
    enqueue_affine_g1(W + o_acc, 4, W + o_out, false, s);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, W + o_out, 4 * G1_BYTES, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        err = hip_err("reading the linear combinations of a step check", e);
        return false;
    }
    return true;
}

bool same_record(const Record& a, const Record& b) {
    return memcmp(a.delta_after, b.delta_after, G1_BYTES) == 0 && memcmp(a.g1_s, b.g1_s, G1_BYTES) == 0 && memcmp(a.g1_sx, b.g1_sx, G1_BYTES) == 0 &&
           memcmp(a.g2_spx, b.g2_spx, G2_BYTES) == 0 && memcmp(a.transcript, b.transcript, HASH_BYTES) == 0 && a.type == b.type && a.params == b.params;
}

// sections `ids` of b are a's byte for byte, and so is the header before delta1; "" or `who` + which section differs from `whose`
std::string same_sections(const Key& a, const Key& b, std::initializer_list<uint32_t> ids, const std::string& who, const std::string& whose) {
    static const char* names[10] = {"", "protocol", "header", "IC", "coefficients", "A", "B1", "B2", "C", "H"};
    for (uint32_t id : ids)
        if (a.secs[id].size != b.secs[id].size || memcmp(a.secs[id].p, b.secs[id].p, a.secs[id].size) != 0)
            return who + "section " + std::to_string(id) + " (" + names[id] + ") differs from " + whose;
    if (memcmp(a.secs[2].p, b.secs[2].p, HDR_DELTA1) != 0)
        return who + "section 2 (header) differs from " + whose + " before delta1 (the sizes, alpha1, beta1, beta2 or gamma2)";
    return "";
}

// what of `next` has to be `prev`'s byte for byte, and the shape of its section 10; "" or what fails
std::string step_structure(const Key& prev, const Key& next) {
    const Section10 &a = prev.s10, &b = next.s10;
    if (b.recs.size() != a.recs.size() + 1)
        return "zkey step: section 10 of the next key has " + std::to_string(b.recs.size()) + " contributions, the previous key " + std::to_string(a.recs.size()) +
               ": exactly one more is expected";
    for (size_t k = 0; k < a.recs.size(); ++k)
        if (!same_record(a.recs[k], b.recs[k])) return "zkey step: section 10: contribution " + std::to_string(k + 1) + " is not the previous key's";
    uint8_t want[HASH_BYTES];
    if (a.blank())
        sections_hash(prev.secs, want);
    else
        memcpy(want, a.cs_hash, HASH_BYTES);
    if (memcmp(want, b.cs_hash, HASH_BYTES) != 0)
        return std::string("zkey step: section 10: the csHash is not ") + (a.blank() ? "the hash of the previous key's sections 1 to 9" : "the previous key's");
    return same_sections(prev, next, {1u, 3u, 4u, 5u, 6u, 7u}, "zkey step: ", "the previous key's");
}

// the caller's 32 bytes, or without them 32 from getrandom()
bool take_seed(const uint8_t* in, uint8_t seed[32]) {
    if (in) {
        memcpy(seed, in, 32);
        return true;
    }
    for (size_t got = 0; got < 32;) {
        const ssize_t k = getrandom(seed + got, 32 - got, 0);
        if (k < 0) return false;
        got += (size_t)k;
    }
    return true;
}

// e(R', delta2') = e(R, delta2) for the sums of step_sums, section 8 before 9; "" or the failure `head` + "8 (C)" + `tail`
std::string sums_rules(const uint8_t* sums, const uint8_t* delta2_prev, const uint8_t* delta2_next, const std::string& head, const std::string& tail,
                       std::vector<PairCheck>& checks) {
    static const char* what[2] = {"8 (C)", "9 (H)"};
    for (int sec = 0; sec < 2; ++sec) {
        const uint8_t *r = sums + 2 * sec * G1_BYTES, *r2 = r + G1_BYTES;
        const std::string msg = head + what[sec] + tail;
        const bool inf = is_zero_bytes(r, G1_BYTES), inf2 = is_zero_bytes(r2, G1_BYTES);
        if (inf != inf2) return msg;
        if (!inf) checks.push_back({r2, delta2_next, r, delta2_prev, msg});  // e(R', delta2') = e(R, delta2)
    }
    return "";
}

int verify_step(const uint8_t* prev_bytes, size_t prev_len, const uint8_t* next_bytes, size_t next_len, const uint8_t* seed_in, gw_status_t* status) {
    std::string err;
    Key prev, next;
    if (!read_key(prev_bytes, prev_len, prev, err)) return fail2(status, "previous key: " + err);
    if (!read_key(next_bytes, next_len, next, err)) return fail2(status, "next key: " + err);
    std::string verdict = step_structure(prev, next);
    if (!verdict.empty()) return fail(status, verdict);
    if (const int rc = cwc_beacon::forms_of(next.s10.recs, next.s10.recs.size() - 1, "zkey", err))  // the new record, if it is a beacon
        return rc == 1 ? fail(status, err) : fail2(status, err);
    uint8_t seed[32];
    if (!take_seed(seed_in, seed)) return fail2(status, "zkey step: getrandom failed");
    const gwb_zkey &zp = *prev.z, &zn = *next.z;
    const Generators gen;
    std::vector<PairCheck> checks;
    uint8_t sp[G2_BYTES];
    if (is_zero_bytes(zp.delta1, G1_BYTES)) return fail(status, "zkey step: delta1 of the previous key is the point at infinity");
    const size_t k = next.s10.recs.size() - 1;
    std::string host_verdict = record_rules(next.s10, k, zp.delta1, sp, checks);
    if (host_verdict.empty()) host_verdict = delta_rules(zn, next.s10.recs[k].delta_after, gen.g1, gen.g2, checks);
    uint8_t sums[4 * G1_BYTES];
    if (host_verdict.empty()) {
        if (is_zero_bytes(zp.delta2, G2_BYTES) || !g2_stored_in_subgroup(zp.delta2))
            host_verdict = "zkey step: delta2 of the previous key is not a point of order r";
    }
    if (host_verdict.empty()) {
        if (!step_sums(zp, zn, seed, sums, err)) return fail2(status, err);
        host_verdict = sums_rules(sums, zp.delta2, zn.delta2, "zkey step: section ", " is not the previous key's section divided by the contribution's secret", checks);
    }
    if (!run_checks(checks, verdict, err)) return fail2(status, err);
    if (verdict.empty()) verdict = host_verdict;
    if (!verdict.empty()) return fail(status, verdict);
    set_ok(status);
    return 0;
}

// ---- the powers check of a `.ptau` and the key check -------------------------------------------------------------------------

// rc and message of a C ABI call, for the callers below
struct Outcome {
    int rc = 0;
    std::string msg;
};
Outcome outcome_of(int rc, gw_status_t& st) {
    Outcome o{rc, st.error_msg ? st.error_msg : ""};
    free(st.error_msg);
    st.error_msg = nullptr;
    return o;
}

// The six sums of the powers check, stored form: g1[5][64] = V, U, V_n, S_A, S_B and g2[128] = S_2, over the first n points of
// sections 3 to 5 and the first `pairs` points of section 2 with the point after each (2n - 1 for a setup's prefixes of the
// domain n, 2n - 2 for a whole file of 2n - 1 points).  T1 goes through the device in two ranges, [0, n) and [n, pairs), so that
// V_n is V's state between them; a piece of m points of a range is uploaded with the point after it, and U's list is the same
// buffer one point on.
bool powers_sums(const cwc_ptau::Plan& pl, uint64_t n, uint64_t pairs, const uint8_t seed[32], uint8_t* g1, uint8_t* g2, std::string& err) {
    const uint64_t chunk = std::max<uint64_t>(1, std::min(chunk_points(), n));
    const uint32_t blocks1 = blocks_for(chunk, LC_THREADS<G1>), blocks2 = blocks_for(chunk, LC_THREADS<G2>);
    Stream s;
    DeviceBuf work;
    Carve cw;
    const size_t o_p0 = cw.take((chunk + 1) * G1_BYTES), o_p1 = cw.take(chunk * G1_BYTES), o_q = cw.take(chunk * G2_BYTES), o_rho = cw.take(chunk * RHO_BYTES),
                 o_part1 = cw.take(2ull * blocks1 * sizeof(Xyzz<G1>)), o_part2 = cw.take((size_t)blocks2 * sizeof(Xyzz<G2>)),
                 o_acc1 = cw.take(5 * sizeof(Xyzz<G1>)), o_acc2 = cw.take(sizeof(Xyzz<G2>)), o_out1 = cw.take(5 * G1_BYTES), o_out2 = cw.take(G2_BYTES);
    hipError_t e = s.create();
    if (e == hipSuccess) e = work.alloc(cw.o);
    if (e == hipSuccess) e = hipMemsetAsync(work.as<uint8_t>() + o_acc1, 0, o_out1 - o_acc1, s);  // the accumulators of both groups
    if (e != hipSuccess) {
        err = hip_err("allocating the powers check's workspace", e);
        return false;
    }
    uint8_t* W = work.as<uint8_t>();
    Xyzz<G1>* acc1 = (Xyzz<G1>*)(W + o_acc1);
    std::vector<uint8_t> rho(chunk * RHO_BYTES);
    // one piece: rho[first .. first + m) on the lists a (m + extra points uploaded) and b (nullptr: a one point on) into acc[0], acc[1]
    auto piece1 = [&](const uint8_t* a, const uint8_t* b, uint64_t first, uint32_t m, Xyzz<G1>* acc) {
        fill_rho(seed, first, m, rho.data());
        e = hipMemcpyAsync(W + o_p0, a + first * G1_BYTES, (size_t)(m + (b ? 0 : 1)) * G1_BYTES, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && b) e = hipMemcpyAsync(W + o_p1, b + first * G1_BYTES, (size_t)m * G1_BYTES, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(W + o_rho, rho.data(), (size_t)m * RHO_BYTES, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return;
        enqueue_lincomb<G1>(W + o_p0, b ? W + o_p1 : W + o_p0 + G1_BYTES, 2, m, false, W + o_rho, (Xyzz<G1>*)(W + o_part1), acc, s);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);  // rho is refilled for the next piece
    };
    const uint64_t ends[2] = {n, pairs};  // T1: V and U over [0, n), V_n = V there, then [n, pairs)
    for (int range = 0; range < 2 && e == hipSuccess; ++range) {
        for (uint64_t at = range ? n : 0; at < ends[range] && e == hipSuccess; at += chunk)
            piece1(pl.t1, nullptr, at, (uint32_t)std::min<uint64_t>(chunk, ends[range] - at), acc1);
        if (range == 0 && e == hipSuccess) e = hipMemcpyAsync(acc1 + 2, acc1, sizeof(Xyzz<G1>), hipMemcpyDeviceToDevice, s);
    }
    for (uint64_t at = 0; at < n && e == hipSuccess; at += chunk) piece1(pl.at, pl.bt, at, (uint32_t)std::min<uint64_t>(chunk, n - at), acc1 + 3);
    for (uint64_t at = 0; at < n && e == hipSuccess; at += chunk) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - at);
        fill_rho(seed, at, m, rho.data());
        e = hipMemcpyAsync(W + o_q, pl.t2 + at * G2_BYTES, (size_t)m * G2_BYTES, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(W + o_rho, rho.data(), (size_t)m * RHO_BYTES, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) break;
        enqueue_lincomb<G2>(W + o_q, W + o_q, 1, m, false, W + o_rho, (Xyzz<G2>*)(W + o_part2), (Xyzz<G2>*)(W + o_acc2), s);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e == hipSuccess) {
        enqueue_affine<G1>(W + o_acc1, 5, W + o_out1, false, s);
        enqueue_affine<G2>(W + o_acc2, 1, W + o_out2, false, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(g1, W + o_out1, 5 * G1_BYTES, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(g2, W + o_out2, G2_BYTES, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        err = hip_err("running the linear combinations of the powers check", e);
        return false;
    }
    return true;
}

}  // namespace

// The six sums (kept in `keep`, which has to outlive the checks) and the five equations of the powers check over the lengths of
// powers_sums; whole: the lengths are a whole file's, and the messages say so.  The equations go to `checks`; host_verdict: the
// first of them that fails without a pairing.
bool cwc_contrib::powers_rules(const cwc_ptau::Plan& pl, uint64_t n, uint64_t pairs, bool whole, const uint8_t seed[32], PowersSums& keep,
                               std::vector<PairCheck>& checks, std::string& host_verdict, std::string& err) {
    if (!powers_sums(pl, n, pairs, seed, keep.g1, keep.s2, err)) return false;
    const Generators gen;
    memcpy(keep.gen1, gen.g1, G1_BYTES);
    memcpy(keep.gen2, gen.g2, G2_BYTES);
    const uint8_t *V = keep.g1, *U = V + G1_BYTES, *Vn = V + 2 * G1_BYTES, *SA = V + 3 * G1_BYTES, *SB = V + 4 * G1_BYTES;
    const uint8_t* t2_1 = pl.t2 + G2_BYTES;
    const std::string first2n = whole ? "the points" : "the first 2n points", firstn = whole ? "the points" : "the first n points";
    const struct {
        const uint8_t *a1, *a2, *b1, *b2;
        std::string msg;
    } eqs[5] = {{U, keep.gen2, V, t2_1, "ptau: section 2 (tauG1): " + first2n + " are not consecutive powers of the tau of section 3"},
                {keep.gen1, keep.s2, Vn, keep.gen2, "ptau: section 3 (tauG2): " + firstn + " are not the powers of the tau of section 2"},
                {SA, keep.gen2, pl.at, keep.s2, "ptau: section 4 (alphaTauG1): " + firstn + " are not alphaTauG1[0] times the powers of tau"},
                {SB, keep.gen2, pl.bt, keep.s2, "ptau: section 5 (betaTauG1): " + firstn + " are not betaTauG1[0] times the powers of tau"},
                {pl.bt, keep.gen2, keep.gen1, pl.beta2, "ptau: section 6 (betaG2): the point is not the G2 generator times the beta of betaTauG1[0]"}};
    for (int i = 0; i < 5 && host_verdict.empty(); ++i) host_verdict = pair_rule(eqs[i].a1, eqs[i].a2, eqs[i].b1, eqs[i].b2, eqs[i].msg, checks);
    return true;
}
bool cwc_contrib::run_pair_checks(const std::vector<PairCheck>& checks, std::string& verdict, std::string& err) { return run_checks(checks, verdict, err); }
bool cwc_contrib::seed_or_draw(const uint8_t* in, uint8_t seed[32]) { return take_seed(in, seed); }

namespace {

// gwb_ptau_check_powers: rc 0, 1 (msg: the verdict) or 2
Outcome check_powers(const uint8_t* data, size_t len, uint32_t domain_power, const uint8_t* seed_in) {
    std::string err;
    cwc_ptau::View view;
    cwc_ptau::Plan pl;
    if (!cwc_ptau::parse(data, len, view, err) || !cwc_ptau::plan(view, domain_power, GWB_PTAU_LAGRANGE_COMPUTE, pl, err) ||
        !cwc_ptau::check_header_points(pl, err) || !cwc_ptau::check_bulk_points(pl, err))
        return {2, err};
    gw_status_t st{};
    Outcome sub = outcome_of(gwb_ptau_check_g2(data, len, domain_power, GWB_PTAU_LAGRANGE_COMPUTE, &st), st);
    if (sub.rc != 0) return {sub.msg.find("order-r subgroup") != std::string::npos ? 1 : 2, sub.msg};  // its other refusals were made above
    uint8_t seed[32];
    if (!take_seed(seed_in, seed)) return {2, "ptau: getrandom failed"};
    PowersSums sums;
    std::vector<PairCheck> checks;
    std::string host_verdict, verdict;
    if (!powers_rules(pl, 1ull << pl.p, (2ull << pl.p) - 1, false, seed, sums, checks, host_verdict, err)) return {2, err};
    if (!run_checks(checks, verdict, err)) return {2, err};
    if (verdict.empty()) verdict = host_verdict;
    return {verdict.empty() ? 0 : 1, verdict};
}

// ---- the Lagrange check of a prepared `.ptau` ------------------------------------------------------------------------------------

// The device side of one Lagrange check: a stream and one workspace sized for the largest level asked for.  rho_i belongs to
// the slot i of a section's all-level layout and is the same in the four sections (every section has an equation of its own).
struct LagrangeDevice {
    Stream s;
    DeviceBuf work;
    uint64_t chunk = 0;
    uint32_t top = 0;
    InvPowersOfTwo inv;
    size_t o_rho = 0, o_x = 0, o_c = 0, o_tw = 0, o_pts = 0, o_part = 0, o_acc = 0, o_out = 0;

    bool open(uint32_t top_level, const uint8_t seed[32], std::string& err) {
        top = top_level;
        const uint64_t slots = (2ull << top) - 1;
        chunk = std::min(chunk_points(), slots);
        Carve cw;
        o_rho = cw.take(slots * RHO_BYTES);
        o_x = cw.take(slots * 32);
        o_c = cw.take((1ull << top) * 32);
        o_tw = cw.take((1ull << (top - 1)) * 32);
        o_pts = cw.take(chunk * G2_BYTES);
        o_part = cw.take((size_t)blocks_for(chunk, LC_THREADS<G2>) * sizeof(Xyzz<G2>));  // more than G1's blocks of 256 need
        o_acc = cw.take(2 * sizeof(Xyzz<G2>));
        o_out = cw.take(2 * G2_BYTES);
        hipError_t e = s.create();
        if (e == hipSuccess) e = work.alloc(cw.o);
        if (e != hipSuccess) {
            err = hip_err("allocating the Lagrange check's workspace", e);
            return false;
        }
        uint8_t* W = work.as<uint8_t>();
        std::vector<uint8_t> rho(slots * RHO_BYTES);
        fill_rho(seed, 0, slots, rho.data());
        Fr wn, g, rm1 = cwc::fr_p();
        qap_roots(top - 1, wn, g);  // g = w_(2^top)
        rm1.v[0] -= 1;
        for (uint32_t m = 0; m <= cwc_ptau::MAX_POWER + 1; ++m) {
            Fr k{{1, 0, 0, 0, 0, 0, 0, 0}};
            if (m >= 1 && m <= 28) cwc::u256_sub(k, cwc::fr_p(), cwc::u256_shr(rm1, m));  // 1 / 2^m = r - (r - 1) / 2^m
            inv.v[m] = cwc::fr_to_mont(k);
        }
        e = hipMemcpyAsync(W + o_rho, rho.data(), rho.size(), hipMemcpyHostToDevice, s);
        hipLaunchKernelGGL(fr_powers_kernel, dim3(blocks_for(1ull << (top - 1), THREADS)), dim3(THREADS), 0, s, (Fr*)(W + o_tw), 1u << (top - 1),
                           powers_of(cwc::fr_inv_fermat(g)));
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);  // the copy has left the host array
        if (e != hipSuccess) err = hip_err("uploading the Lagrange check's scalars", e);
        return e == hipSuccess;
    }

    // acc += sum scalar_i P_i over the n stored points at host address p, in pieces; the scalars are on the device
    template <class T, uint32_t WORDS>
    hipError_t sum(const uint8_t* p, uint64_t n, const uint8_t* d_scalars, Xyzz<T>* acc) {
        uint8_t* W = work.as<uint8_t>();
        hipError_t e = hipSuccess;
        for (uint64_t at = 0; at < n && e == hipSuccess; at += chunk) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - at);
            e = hipMemcpyAsync(W + o_pts, p + at * POINT_BYTES<T>, (size_t)m * POINT_BYTES<T>, hipMemcpyHostToDevice, s);
            if (e != hipSuccess) break;
            enqueue_lincomb<T, WORDS>(W + o_pts, W + o_pts, 1, m, false, d_scalars + at * (4 * WORDS), (Xyzz<T>*)(W + o_part), acc, s);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(s);  // the piece's buffer is written again by the next upload
        }
        return e;
    }

    // sum_{m in [m_lo, m_hi]} sum_k rho_{m,k} Lag_m[k] over section id against sum_i c_i T_i over section id - 10; `equal`: the verdict
    template <class T>
    bool levels(const cwc_ptau::View& v, uint32_t id, uint32_t m_lo, uint32_t m_hi, bool& equal, std::string& err) {
        uint8_t* W = work.as<uint8_t>();
        const uint32_t lo = (1u << m_lo) - 1u, hi = (2u << m_hi) - 1u;
        const uint64_t n_right = (1ull << m_hi) - (id == 12 && m_hi == v.power + 1 ? 1 : 0);  // c_{2n-1} multiplies O: dropped
        Xyzz<T>* acc = (Xyzz<T>*)(W + o_acc);
        Fr *x = (Fr*)(W + o_x), *c = (Fr*)(W + o_c);
        hipError_t e = hipMemsetAsync(acc, 0, 2 * sizeof(Xyzz<T>), s);
        if (e == hipSuccess) e = sum<T, 4>(v.sec[id].p + (size_t)lo * POINT_BYTES<T>, hi - lo, W + o_rho + (size_t)lo * RHO_BYTES, acc);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(rho_levels_kernel, dim3(blocks_for(hi - lo, THREADS)), dim3(THREADS), 0, s, (const uint32_t*)(W + o_rho), lo, hi, x);
            for (uint32_t st = 0; st < m_hi; ++st)
                hipLaunchKernelGGL(fr_levels_stage_kernel, dim3(blocks_for(1ull << m_hi, THREADS)), dim3(THREADS), 0, s, x, m_hi, st, m_lo, top - 1 - st,
                                   (const Fr*)(W + o_tw));
            hipLaunchKernelGGL(fold_levels_kernel, dim3(blocks_for(1ull << m_hi, THREADS)), dim3(THREADS), 0, s, (const Fr*)x, m_lo, m_hi, inv, c);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = sum<T, 8>(v.sec[id - 10].p, n_right, (const uint8_t*)c, acc + 1);
        uint8_t out[2 * G2_BYTES];
        if (e == hipSuccess) {
            enqueue_affine<T>(acc, 2, W + o_out, false, s);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out, W + o_out, 2 * POINT_BYTES<T>, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            err = hip_err("running the linear combinations of the Lagrange check", e);
            return false;
        }
        equal = memcmp(out, out + POINT_BYTES<T>, POINT_BYTES<T>) == 0;
        return true;
    }
    bool levels(const cwc_ptau::View& v, uint32_t id, uint32_t m_lo, uint32_t m_hi, bool& equal, std::string& err) {
        return id == 13 ? levels<G2>(v, id, m_lo, m_hi, equal, err) : levels<G1>(v, id, m_lo, m_hi, equal, err);
    }
};

// gwb_ptau_check_lagrange: rc 0, 1 (msg: the verdict) or 2
Outcome check_lagrange(const uint8_t* data, size_t len, uint32_t domain_power, const uint8_t* seed_in) {
    std::string err;
    cwc_ptau::View view;
    if (!cwc_ptau::parse(data, len, view, err)) return {2, err};
    const bool all = domain_power == GWB_PTAU_ALL_LEVELS;
    struct Job {
        uint32_t id, m_lo, m_hi;
    };
    std::vector<Job> jobs;
    if (all) {
        if (!cwc_ptau::need_prepared(view, err)) return {2, err};
        for (uint32_t id = 12; id <= 15; ++id) jobs.push_back({id, 0, cwc_ptau::top_level(view, id)});
    } else {
        cwc_ptau::Plan pl;
        if (!cwc_ptau::plan(view, domain_power, GWB_PTAU_LAGRANGE_FILE, pl, err) || !cwc_ptau::check_header_points(pl, err)) return {2, err};
        const uint32_t p = domain_power;
        jobs = {{12, p, p}, {12, p + 1, p + 1}, {13, p, p}, {14, p, p}, {15, p, p}};
    }
    const uint32_t top = all ? view.power + 1 : domain_power + 1;
    if (top > MAX_DOMAIN_POWER + 1)
        return {2, "ptau: the Lagrange check of level " + std::to_string(top) + " needs a root of unity of order 2^" + std::to_string(top) + ", which r does not have"};
    for (const Job& j : jobs)
        if (!cwc_ptau::check_lagrange_points(view, j.id, j.m_lo, j.m_hi, err)) return {2, err};
    for (const Job& j : jobs) {  // the equality below sees a small-order component with probability 1 / order only
        if (j.id != 13) continue;
        const uint64_t lo = (1ull << j.m_lo) - 1, hi = (2ull << j.m_hi) - 1;
        const int rc = cwc_ptau::check_g2_points(13, lo, view.sec[13].p + lo * G2_BYTES, hi - lo, err);
        if (rc != 0) return {rc, err};
    }
    uint8_t seed[32];
    if (!take_seed(seed_in, seed)) return {2, "ptau: getrandom failed"};  // drawn after the file is seen
    LagrangeDevice D;
    if (!D.open(top, seed, err)) return {2, err};
    for (const Job& j : jobs) {
        bool equal = false;
        if (!D.levels(view, j.id, j.m_lo, j.m_hi, equal, err)) return {2, err};
        if (equal) continue;
        const std::string who = "ptau: section " + std::to_string(j.id) + " (" + cwc_ptau::section_name(j.id) + ")";
        const std::string what = " not hold the Lagrange forms of section " + std::to_string(j.id - 10);
        if (j.m_lo == j.m_hi) return {1, who + " level " + std::to_string(j.m_lo) + " does" + what};
        for (uint32_t m = j.m_lo; m <= j.m_hi; ++m) {  // which level: one by one, after the verdict is known
            if (!D.levels(view, j.id, m, m, equal, err)) return {2, err};
            if (!equal) return {1, who + " does" + what + ": level " + std::to_string(m) + " is the first that does not"};
        }
        return {1, who + " does" + what};
    }
    return {0, ""};
}

// a verdict of the functions that the contribution check shares with the key check, under the key check's name
std::string as_key_verdict(const std::string& msg) { return msg.compare(0, 6, "zkey: ") == 0 ? "zkey verify: " + msg.substr(6) : msg; }

PhaseTimes<3> g_key_phases;  // remake, linear combinations, pairings: host clock around the three synchronous parts

float ms_since(const std::chrono::steady_clock::time_point& t0) {
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

Outcome verify_key(const uint8_t* zkey, size_t len, gwb_r1cs* r, const uint8_t* ptau, size_t ptau_len, uint32_t mode, uint32_t flags, const uint8_t* seed_in,
                   uint8_t* hashes_out, size_t* n_io) {
    std::string err;
    // 1. parse
    Key key;
    if (!read_key(zkey, len, key, err)) return {2, err};
    if (!(flags & GWB_VERIFY_KEY_SKIP_RECORDS)) {
        const int rc = cwc_beacon::forms_of(key.s10.recs, 0, "zkey", err);
        if (rc != 0) return {rc, rc == 1 ? as_key_verdict(err) : err};
    }
    gw_status_t st{};
    gwb_r1cs_qap_info_t qi;
    if (gwb_r1cs_qap_info(r, &qi, &st) != 0) return {2, outcome_of(1, st).msg};
    {
        cwc_ptau::View view;
        cwc_ptau::Plan pl;
        if (!cwc_ptau::parse(ptau, ptau_len, view, err) || !cwc_ptau::plan(view, qi.domain_power, mode, pl, err) || !cwc_ptau::check_header_points(pl, err))
            return {2, err};
    }
    // 2. sizes
    const gwb_zkey& z = *key.z;
    const uint64_t want[3] = {r->info.n_wires, (uint64_t)r->info.n_pub_out + r->info.n_pub_in, qi.domain_size};
    const uint64_t have[3] = {z.info.n_vars, z.info.n_public, z.info.domain_size};
    static const char* size_names[3] = {"nVars", "nPublic", "domainSize"};
    for (int i = 0; i < 3; ++i)
        if (have[i] != want[i])
            return {1, std::string("zkey verify: ") + size_names[i] + " of the key is " + std::to_string(have[i]) + ", the circuit's is " + std::to_string(want[i])};
    uint8_t seed[32];
    if (!take_seed(seed_in, seed)) return {2, "zkey verify: getrandom failed"};
    // 3. the powers check
    if (flags & GWB_VERIFY_KEY_CHECK_PTAU) {
        const Outcome o = check_powers(ptau, ptau_len, qi.domain_power, seed);
        if (o.rc != 0) return o;
    }
    // 4. the key of the circuit and the file with delta = 1
    auto t0 = std::chrono::steady_clock::now();
    float ms[3] = {0, 0, 0};
    const uint8_t one[32] = {1};
    void* remade = nullptr;
    size_t remade_len = 0;
    if (gwb_groth16_setup_ptau(r, ptau, ptau_len, one, mode, &remade, &remade_len, &st) != 0) return {2, outcome_of(2, st).msg};
    free(st.error_msg);
    st.error_msg = nullptr;
    struct Release {
        void* p;
        ~Release() { gwb_groth16_setup_free(p); }
    } release{remade};
    Key key0;
    if (!read_key(remade, remade_len, key0, err)) return {2, "zkey verify: the remade key: " + err};
    ms[0] = ms_since(t0);
    // 5. structure
    if (gwb_zkey_check_r1cs(key.z.get(), r, &st) != 0) return {1, as_key_verdict(outcome_of(1, st).msg)};
    free(st.error_msg);
    st.error_msg = nullptr;
    std::string verdict = same_sections(key0, key, {1u, 3u, 5u, 6u, 7u}, "zkey verify: ", "the key remade from the circuit and the powers-of-tau file");
    if (!verdict.empty()) return {1, verdict};
    // 6 to 8: host rules in order, their pairings in one launch
    const Section10& s = key.s10;
    const size_t n = s.recs.size();
    const Generators gen;
    std::vector<PairCheck> checks;
    std::vector<uint8_t> sp(std::max<size_t>(n, 1) * G2_BYTES);
    std::string host_verdict;
    if (!(flags & GWB_VERIFY_KEY_SKIP_RECORDS)) {
        if (!s.blank()) {
            uint8_t want_hash[HASH_BYTES];
            sections_hash(key0.secs, want_hash);
            if (memcmp(want_hash, s.cs_hash, HASH_BYTES) != 0)
                host_verdict = "zkey verify: section 10: the csHash is not the hash of sections 1 to 9 of the remade key";
        }
        for (size_t k = 0; k < n && host_verdict.empty(); ++k)
            host_verdict = record_rules(s, k, k ? s.recs[k - 1].delta_after : gen.g1, sp.data() + k * G2_BYTES, checks);
        if (host_verdict.empty()) host_verdict = delta1_rule(z, n ? s.recs[n - 1].delta_after : nullptr, gen.g1);
    }
    if (host_verdict.empty() && is_zero_bytes(z.delta1, G1_BYTES)) host_verdict = "zkey verify: delta1 is the point at infinity";
    if (host_verdict.empty()) host_verdict = delta2_rules(z, gen.g1, gen.g2, checks);
    uint8_t sums[4 * G1_BYTES];
    if (host_verdict.empty()) {
        t0 = std::chrono::steady_clock::now();
        if (!step_sums(*key0.z, z, seed, sums, err)) return {2, err};
        ms[1] = ms_since(t0);
        host_verdict = sums_rules(sums, key0.z->delta2, z.delta2, "zkey verify: section ", " is not the remade key's section divided by delta", checks);
    }
    t0 = std::chrono::steady_clock::now();
    if (!run_checks(checks, verdict, err)) return {2, err};
    ms[2] = ms_since(t0);
    if (verdict.empty()) verdict = host_verdict;
    if (!verdict.empty()) return {1, as_key_verdict(verdict)};
    g_key_phases.store(ms, true);
    const size_t room = *n_io;
    *n_io = n;
    for (size_t k = 0; k < n && k < room && hashes_out; ++k) record_hash(s.recs[k], hashes_out + k * HASH_BYTES);
    return {0, ""};
}

int finish(const Outcome& o, gw_status_t* status) {
    if (o.rc == 0) {
        set_ok(status);
        return 0;
    }
    set_status(status, o.msg);
    return o.rc;
}

// the aid of the linear-combination kernels for one group (the extern functions below)
template <class T, uint32_t WORDS>
int lincomb_aid(const char* fn, const void* d_points, const void* d_rho, size_t n, uint32_t form, void* d_out, void* hip_stream, gw_status_t* status) {
    if (form != GWB_FORM_CANONICAL && form != GWB_FORM_MONTGOMERY) return fail(status, std::string(fn) + ": unknown form " + std::to_string(form));
    const bool canonical = form == GWB_FORM_CANONICAL;
    if (!d_out || (n && (!d_points || !d_rho))) return fail(status, std::string(fn) + ": NULL argument");
    if (n > 0x7fffffffull) return fail(status, std::string(fn) + ": n above 2^31 - 1");
    hipStream_t s = (hipStream_t)hip_stream;
    Carve cw;
    const size_t o_part = cw.take((size_t)blocks_for(n, LC_THREADS<T>) * sizeof(Xyzz<T>)), o_acc = cw.take(sizeof(Xyzz<T>));
    void* ws = nullptr;
    hipError_t e = hipMallocAsync(&ws, cw.o, s);
    if (e != hipSuccess) return fail(status, hip_err("allocating the linear combination's workspace", e));
    uint8_t* W = (uint8_t*)ws;
    e = hipMemsetAsync(W + o_acc, 0, sizeof(Xyzz<T>), s);
    if (e == hipSuccess && n)
        enqueue_lincomb<T, WORDS>((const uint8_t*)d_points, (const uint8_t*)d_points, 1, (uint32_t)n, canonical, (const uint8_t*)d_rho, (Xyzz<T>*)(W + o_part),
                           (Xyzz<T>*)(W + o_acc), s);
    if (e == hipSuccess) {
        enqueue_affine<T>(W + o_acc, 1, (uint8_t*)d_out, canonical, s);
        e = hipGetLastError();
    }
    const hipError_t ef = hipFreeAsync(ws, s);
    if (e != hipSuccess) return fail(status, hip_err("launching the linear combination", e));
    if (ef != hipSuccess) return fail(status, hip_err("releasing the linear combination's workspace", ef));
    set_ok(status);
    return 0;
}

}  // namespace

extern "C" {

int gwb_groth16_contribute(const void* zkey, size_t len, const char* name, const uint8_t* delta, void** out, size_t* out_len, void* hash64,
                           gw_status_t* status) {
    if (!out || !out_len || !hash64 || (!zkey && len)) return fail(status, "gwb_groth16_contribute: NULL argument");
    *out = nullptr;
    *out_len = 0;
    try {
        return contribute((const uint8_t*)zkey, len, name, delta, out, out_len, (uint8_t*)hash64, status);
    } catch (const std::bad_alloc&) {
        return fail(status, "groth16 contribute: out of host memory");
    }
}

int gwb_groth16_beacon(const void* zkey, size_t len, const char* name, const void* beacon_hash, size_t hash_len, uint32_t iterations_exp, void** out,
                       size_t* out_len, void* hash64, gw_status_t* status) {
    if (!out || !out_len || !hash64 || (!zkey && len) || (!beacon_hash && hash_len)) return fail2(status, "gwb_groth16_beacon: NULL argument");
    *out = nullptr;
    *out_len = 0;
    try {
        return beacon((const uint8_t*)zkey, len, name, (const uint8_t*)beacon_hash, hash_len, iterations_exp, out, out_len, (uint8_t*)hash64, status);
    } catch (const std::bad_alloc&) {
        return fail2(status, "beacon: out of host memory");
    }
}

int gwb_groth16_contribute_phase_ms(float* ms) { return g_phases.read(ms); }

int gwb_zkey_verify_contributions(const void* zkey, size_t len, void* hashes_out, size_t* n, gw_status_t* status) {
    if (!n || (!zkey && len) || (*n && !hashes_out)) return fail2(status, "gwb_zkey_verify_contributions: NULL argument");
    try {
        return verify_contributions((const uint8_t*)zkey, len, (uint8_t*)hashes_out, n, status);
    } catch (const std::bad_alloc&) {
        return fail2(status, "zkey: out of host memory");
    }
}

int gwb_zkey_verify_step(const void* prev, size_t prev_len, const void* next, size_t next_len, const uint8_t* seed, gw_status_t* status) {
    if ((!prev && prev_len) || (!next && next_len)) return fail2(status, "gwb_zkey_verify_step: NULL argument");
    try {
        return verify_step((const uint8_t*)prev, prev_len, (const uint8_t*)next, next_len, seed, status);
    } catch (const std::bad_alloc&) {
        return fail2(status, "zkey: out of host memory");
    }
}

int gwb_ptau_check_powers(const void* data, size_t len, uint32_t domain_power, const uint8_t* seed, gw_status_t* status) {
    if (!data && len) return fail2(status, "gwb_ptau_check_powers: NULL argument");
    try {
        return finish(check_powers((const uint8_t*)data, len, domain_power, seed), status);
    } catch (const std::bad_alloc&) {
        return fail2(status, "ptau: out of host memory");
    }
}

int gwb_zkey_verify_key(const void* zkey, size_t len, gwb_r1cs_t* r, const void* ptau, size_t ptau_len, uint32_t lagrange_mode, uint32_t flags,
                        const uint8_t* seed, void* hashes_out, size_t* n, gw_status_t* status) {
    if (!n || !r || (!zkey && len) || (!ptau && ptau_len) || (*n && !hashes_out)) return fail2(status, "gwb_zkey_verify_key: NULL argument");
    if (flags & ~(uint32_t)(GWB_VERIFY_KEY_SKIP_RECORDS | GWB_VERIFY_KEY_CHECK_PTAU)) return fail2(status, "gwb_zkey_verify_key: unknown flags " + std::to_string(flags));
    try {
        return finish(verify_key((const uint8_t*)zkey, len, r, (const uint8_t*)ptau, ptau_len, lagrange_mode, flags, seed, (uint8_t*)hashes_out, n), status);
    } catch (const std::bad_alloc&) {
        return fail2(status, "zkey: out of host memory");
    }
}

int gwb_zkey_verify_key_phase_ms(float* ms) { return g_key_phases.read(ms); }

int gwb_bn254_g1_scale_batch_device(const void* d_points, size_t n, const uint8_t* k32, void* d_out, void* hip_stream, gw_status_t* status) {
    if (!k32 || (n && (!d_points || !d_out))) return fail(status, "gwb_bn254_g1_scale_batch_device: NULL argument");
    if (n > 0x7fffffffull) return fail(status, "gwb_bn254_g1_scale_batch_device: n above 2^31 - 1");
    if (n == 0) {
        set_ok(status);
        return 0;
    }
    Fr k;
    memcpy(k.v, k32, 32);
    hipStream_t s = (hipStream_t)hip_stream;
    Carve cw;
    const size_t o_x = cw.take(n * sizeof(Xyzz<G1>)), o_k = cw.take(32);
    void* ws = nullptr;
    hipError_t e = hipMallocAsync(&ws, cw.o, s);
    if (e != hipSuccess) return fail(status, hip_err("allocating the scaling workspace", e));
    uint8_t* W = (uint8_t*)ws;
    hipLaunchKernelGGL(put_scalar_kernel, dim3(1), dim3(64), 0, s, (Fr*)(W + o_k), k);
    hipLaunchKernelGGL(scale_points_kernel, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, s, (const uint8_t*)d_points, (uint32_t)n, 1u, (const Fr*)(W + o_k),
                       (Xyzz<G1>*)(W + o_x));
    enqueue_affine_g1(W + o_x, (uint32_t)n, (uint8_t*)d_out, true, s);
    e = hipGetLastError();
    const hipError_t ef = hipFreeAsync(ws, s);
    if (e != hipSuccess) return fail(status, hip_err("launching the scaling", e));
    if (ef != hipSuccess) return fail(status, hip_err("releasing the scaling workspace", ef));
    set_ok(status);
    return 0;
}

int gwb_bn254_g1_lincomb128_device(const void* d_points, const void* d_rho, size_t n, void* d_out, void* hip_stream, gw_status_t* status) {
    return lincomb_aid<G1, 4>("gwb_bn254_g1_lincomb128_device", d_points, d_rho, n, GWB_FORM_CANONICAL, d_out, hip_stream, status);
}

int gwb_bn254_g2_lincomb128_device(const void* d_points, const void* d_rho, size_t n, void* d_out, void* hip_stream, gw_status_t* status) {
    return lincomb_aid<G2, 4>("gwb_bn254_g2_lincomb128_device", d_points, d_rho, n, GWB_FORM_CANONICAL, d_out, hip_stream, status);
}

int gwb_bn254_g1_lincomb_device(const void* d_points, const void* d_scalars, size_t n, uint32_t form, void* d_out, void* hip_stream, gw_status_t* status) {
    return lincomb_aid<G1, 8>("gwb_bn254_g1_lincomb_device", d_points, d_scalars, n, form, d_out, hip_stream, status);
}

int gwb_bn254_g2_lincomb_device(const void* d_points, const void* d_scalars, size_t n, uint32_t form, void* d_out, void* hip_stream, gw_status_t* status) {
    return lincomb_aid<G2, 8>("gwb_bn254_g2_lincomb_device", d_points, d_scalars, n, form, d_out, hip_stream, status);
}

int gwb_ptau_check_lagrange(const void* data, size_t len, uint32_t domain_power, const uint8_t* seed, gw_status_t* status) {
    if (!data && len) return fail2(status, "gwb_ptau_check_lagrange: NULL argument");
    try {
        return finish(check_lagrange((const uint8_t*)data, len, domain_power, seed), status);
    } catch (const std::bad_alloc&) {
        return fail2(status, "ptau: out of host memory");
    }
}

}  // extern "C"
