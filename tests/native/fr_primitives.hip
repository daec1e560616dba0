// Device harness of tests/test_gpu_fr_primitives.py (gfx950): runs the field primitives of csrc/fr_gfx950.hpp and
// r1cs/fq_gfx950.hpp, each as the product calls it, in full 64-lane waves on operand records read from a file, and writes the
// raw result limbs to a file.  It holds no expected values: the test compares with Python big integers.
//
//   fr_primitives IN OUT
//   IN  = sections { u32 op, n, in_words, out_words, param; u32 data[n * in_words] }   (n: records = lanes, a multiple of 64;
//         for the cooperative ops one record per LANE GROUP, n * 4 lanes)
//   OUT = the sections' results back to back, n * out_words u32 each
//
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I circom-witnesscalc_amd/csrc -I circom-witnesscalc_amd/r1cs
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "fr_gfx950.hpp"
#include "fq_gfx950.hpp"

using namespace cwc;
using namespace cwc_g16;

enum Op : uint32_t {
    OP_FR_MUL = 1, OP_FR_MUL_WAVE, OP_FR_SQR, OP_FR_TO_MONT, OP_FR_FROM_MONT, OP_FR_ADD, OP_FR_SUB, OP_FR_ADD_WAVE, OP_FR_SUB_WAVE,
    OP_FR_ADDSUB_WAVE, OP_FR_NEG, OP_FR_MUL_CHAIN, OP_FR_MUL_WAVE_CHAIN,
    OP_FQ_MUL = 20, OP_FQ_ADD, OP_FQ_SUB, OP_FQ_NEG, OP_FQ_TO_MONT, OP_FQ_FROM_MONT, OP_FQ_MUL_CHAIN,
    OP_FR_INV = 30,
    OP_DIV_DIGITS = 40, OP_DIV_SHORT, OP_DIV_2BY1, OP_DIV_RECIP, OP_DIV_3BY2, OP_DIV_128,
    OP_COOP4 = 50, OP_COOP4R, OP_ADDSUB_COOP4, OP_COOP4_CHAIN, OP_COOP4_FUSED_CHAIN,
};

__device__ __forceinline__ Fr ld(const uint32_t* p) {
    Fr x;
#pragma unroll
    for (int i = 0; i < 8; ++i) x.v[i] = p[i];
    return x;
}
__device__ __forceinline__ void st(uint32_t* p, const Fr& x) {
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = x.v[i];
}
__device__ __forceinline__ uint64_t ld64(const uint32_t* p) { return ((uint64_t)p[1] << 32) | p[0]; }
__device__ __forceinline__ void st64(uint32_t* p, uint64_t x) {
    p[0] = (uint32_t)x;
    p[1] = (uint32_t)(x >> 32);
}
__device__ __forceinline__ bool wave_any(bool p) { return __ballot(p) != 0ull; }

// one record per lane; n is a multiple of 64, so every wave is full or absent.  (Workgroups of four waves, one per SIMD: the asm blocks
// name VGPRs up to v191 like the interpreter's kernels, which the default bound of 1024 threads would put out of reach.)
template <uint32_t OP, uint32_t IW, uint32_t OW>
__global__ void __launch_bounds__(256) lane_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, uint32_t param) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t* r = in + (size_t)t * IW;
    uint32_t* o = out + (size_t)t * OW;
    Fr pv = fr_p();  // the modulus in VGPRs, as the interpreter holds it
#pragma unroll
    for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(pv.v[i]));
    if constexpr (OP == OP_FR_MUL) st(o, fr_mul(ld(r), ld(r + 8)));
    if constexpr (OP == OP_FR_MUL_WAVE) st(o, fr_mul_wave(ld(r), ld(r + 8), pv));
    if constexpr (OP == OP_FR_SQR) st(o, fr_sqr(ld(r)));
    if constexpr (OP == OP_FR_TO_MONT) st(o, fr_to_mont(ld(r)));
    if constexpr (OP == OP_FR_FROM_MONT) st(o, fr_from_mont(ld(r)));
    if constexpr (OP == OP_FR_ADD) st(o, fr_add(ld(r), ld(r + 8)));
    if constexpr (OP == OP_FR_SUB) st(o, fr_sub(ld(r), ld(r + 8)));
    if constexpr (OP == OP_FR_ADD_WAVE) st(o, fr_add_wave(ld(r), ld(r + 8), pv));
    if constexpr (OP == OP_FR_SUB_WAVE) st(o, fr_sub_wave(ld(r), ld(r + 8), pv));
    if constexpr (OP == OP_FR_ADDSUB_WAVE) {
        const uint32_t sub = r[16];
        const unsigned long long subm = __ballot(sub == 1u);
        st(o, fr_addsub_wave(ld(r), ld(r + 8), pv, sub == 1u ? ~0u : 0u, subm, ~subm));
    }
    if constexpr (OP == OP_FR_NEG) st(o, fr_neg(ld(r)));
    if constexpr (OP == OP_FR_MUL_CHAIN || OP == OP_FR_MUL_WAVE_CHAIN || OP == OP_FQ_MUL_CHAIN) {  // b <- a * b, param times; the first eight and the last kept
        const Fr a = ld(r);
        Fr b = ld(r + 8);
        for (uint32_t i = 0; i < param; ++i) {
            if constexpr (OP == OP_FR_MUL_CHAIN) b = fr_mul(a, b);
            if constexpr (OP == OP_FR_MUL_WAVE_CHAIN) b = fr_mul_wave(a, b, pv);
            if constexpr (OP == OP_FQ_MUL_CHAIN) b = fq_mul(a, b);
            if (i < 8) st(o + 8 * i, b);
        }
        st(o + 64, b);
    }
    if constexpr (OP == OP_FQ_MUL) st(o, fq_mul(ld(r), ld(r + 8)));
    if constexpr (OP == OP_FQ_ADD) st(o, fq_add(ld(r), ld(r + 8)));
    if constexpr (OP == OP_FQ_SUB) st(o, fq_sub(ld(r), ld(r + 8)));
    if constexpr (OP == OP_FQ_NEG) st(o, fq_neg(ld(r)));
    if constexpr (OP == OP_FQ_TO_MONT) st(o, fq_to_mont(ld(r)));
    if constexpr (OP == OP_FQ_FROM_MONT) st(o, fq_from_mont(ld(r)));
    if constexpr (OP == OP_FR_INV) st(o, fr_inv(ld(r)));
    if constexpr (OP == OP_DIV_DIGITS) {  // digits and bitlen_b as the interpreter's Idiv / Mod bundles derive them (wave-wide maximum)
        const Fr x = ld(r), ys = ld(r + 8);
        const uint32_t lx = u256_bitlen(x), ly = u256_bitlen(ys);
        const uint32_t my_dig = lx >= ly ? (lx - ly + 32u) >> 5 : 0u;
        uint32_t dig = 0;
#pragma unroll
        for (uint32_t dd = 1; dd <= 8; ++dd) dig = wave_any(my_dig >= dd) ? dd : dig;
        Fr q, rem;
        u256_divrem_digits(q, rem, x, ys, dig, ly);
        st(o, q);
        st(o + 8, rem);
    }
    if constexpr (OP == OP_DIV_SHORT || OP == OP_DIV_128) {
        Fr q, rem;
        if constexpr (OP == OP_DIV_SHORT) u128_divrem_64(q, rem, ld(r), ld(r + 8));
        if constexpr (OP == OP_DIV_128) u256_divrem_128(q, rem, ld(r), ld(r + 8));
        st(o, q);
        st(o + 8, rem);
    }
    if constexpr (OP == OP_DIV_2BY1) {  // (u1, u0, dn): u1 < dn, dn normalised -> (q, r, v)
        const uint64_t u1 = ld64(r), u0 = ld64(r + 2), dn = ld64(r + 4), v = recip64(dn);
        uint64_t q, rem;
        div2by1(u1, u0, dn, v, q, rem);
        st64(o, q);
        st64(o + 2, rem);
        st64(o + 4, v);
    }
    if constexpr (OP == OP_DIV_RECIP) {  // (th, tl, d, high) -> (qh, ql, rem)
        const uint64_t th = ld64(r), tl = ld64(r + 2), d = ld64(r + 4);
        const uint32_t s = clz64_nonzero(d);
        const uint64_t dn = d << s, v = recip64(dn);
        uint64_t qh, ql, rem;
        u128_divrem_64_recip(th, tl, d, s, dn, v, r[6] != 0u, qh, ql, rem);
        st64(o, qh);
        st64(o + 2, ql);
        st64(o + 4, rem);
    }
    if constexpr (OP == OP_DIV_3BY2) {  // (u2, u1, u0, d1, d0): (u2:u1) < (d1:d0), d1 normalised -> (q, r1, r0, v)
        const uint64_t u2 = ld64(r), u1 = ld64(r + 2), u0 = ld64(r + 4), d1 = ld64(r + 6), d0 = ld64(r + 8);
        const uint64_t v = recip64_3by2(d1, d0);
        uint64_t q, r1, r0;
        div3by2(u2, u1, u0, d1, d0, v, q, r1, r0);
        st64(o, q);
        st64(o + 2, r1);
        st64(o + 4, r0);
        st64(o + 6, v);
    }
}

// one record per group of four lanes; lane 4v + q holds all of a, limbs 2q and 2q + 1 of the other operands and of r
template <uint32_t OP, uint32_t IW, uint32_t OW>
__global__ void __launch_bounds__(256) coop_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n_groups, uint32_t param) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 4u * n_groups) return;   // (n_groups is a multiple of 16: whole waves)
    const uint32_t g = t >> 2, cq = t & 3u;
    const uint32_t* r = in + (size_t)g * IW;
    uint32_t* o = out + (size_t)g * OW + 2u * cq;
    uint32_t nq0 = cq == 0 ? CWC_P0 : cq == 1 ? CWC_P2 : cq == 2 ? CWC_P4 : CWC_P6;
    uint32_t nq1 = cq == 0 ? CWC_P1 : cq == 1 ? CWC_P3 : cq == 2 ? CWC_P5 : CWC_P7;
    asm volatile("" : "+v"(nq0), "+v"(nq1));
    uint32_t res[2];
    if constexpr (OP == OP_COOP4) {
        fr_mul_coop4(ld(r), r[8 + 2 * cq], r[9 + 2 * cq], nq0, nq1, res);
        o[0] = res[0]; o[1] = res[1];
    }
    if constexpr (OP == OP_COOP4R) {
        fr_mul_coop4r(ld(r), r[2 * cq], r[1 + 2 * cq], r[8 + 2 * cq], r[9 + 2 * cq], nq0, nq1, r[16], res);
        o[0] = res[0]; o[1] = res[1];
    }
    if constexpr (OP == OP_ADDSUB_COOP4) {
        fr_addsub_coop4(r[2 * cq], r[1 + 2 * cq], r[8 + 2 * cq], r[9 + 2 * cq], nq0, nq1, r[16], res);
        o[0] = res[0]; o[1] = res[1];
    }
    if constexpr (OP == OP_COOP4_CHAIN) {  // b <- a * b, param times
        const Fr a = ld(r);
        uint32_t b0 = r[8 + 2 * cq], b1 = r[9 + 2 * cq];
        for (uint32_t i = 0; i < param; ++i) {
            fr_mul_coop4(a, b0, b1, nq0, nq1, res);
            b0 = res[0]; b1 = res[1];
            if (i < 8) { o[8 * i] = b0; o[8 * i + 1] = b1; }
        }
        o[64] = b0; o[65] = b1;
    }
    if constexpr (OP == OP_COOP4_FUSED_CHAIN) {
        // the fused narrow bundle's pattern (class C_MULF), param rounds: acc = a * acc; acc = x2 * acc (the running value as the
        // lanes hold it, the other factor in full); acc = acc + x3; acc = acc - x4; acc = x5 - acc.  Record: a, acc, x2..x5.
        const Fr a = ld(r), x2 = ld(r + 16);
        uint32_t a0 = r[8 + 2 * cq], a1 = r[9 + 2 * cq];
        const uint32_t x30 = r[24 + 2 * cq], x31 = r[25 + 2 * cq], x40 = r[32 + 2 * cq], x41 = r[33 + 2 * cq], x50 = r[40 + 2 * cq], x51 = r[41 + 2 * cq];
        uint32_t step = 0;
        auto keep = [&]() {
            if (step < 10) { o[8 * step] = a0; o[8 * step + 1] = a1; }
            ++step;
        };
        for (uint32_t i = 0; i < param; ++i) {
            fr_mul_coop4(a, a0, a1, nq0, nq1, res);
            a0 = res[0]; a1 = res[1]; keep();
            fr_mul_coop4(x2, a0, a1, nq0, nq1, res);
            a0 = res[0]; a1 = res[1]; keep();
            fr_addsub_coop4(a0, a1, x30, x31, nq0, nq1, 0u, res);
            a0 = res[0]; a1 = res[1]; keep();
            fr_addsub_coop4(a0, a1, x40, x41, nq0, nq1, 1u, res);
            a0 = res[0]; a1 = res[1]; keep();
            fr_addsub_coop4(x50, x51, a0, a1, nq0, nq1, 1u, res);
            a0 = res[0]; a1 = res[1]; keep();
        }
        o[80] = a0; o[81] = a1;
    }
}

#define HIP_OK(x)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                        \
            return 3;                                                                      \
        }                                                                                  \
    } while (0)

template <uint32_t OP, uint32_t IW, uint32_t OW, bool COOP>
static int launch(const uint32_t* din, uint32_t* dout, uint32_t n, uint32_t iw, uint32_t ow, uint32_t param) {
    if (iw != IW || ow != OW) {
        fprintf(stderr, "op %u: record of %u -> %u words, expected %u -> %u\n", OP, iw, ow, IW, OW);
        return 2;
    }
    const uint32_t lanes = COOP ? 4u * n : n;
    const uint32_t block = 256;  // four waves per workgroup
    if constexpr (COOP) coop_kernel<OP, IW, OW><<<(lanes + block - 1) / block, block>>>(din, dout, n, param);
    else lane_kernel<OP, IW, OW><<<(lanes + block - 1) / block, block>>>(din, dout, n, param);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    return 0;
}

static int dispatch(uint32_t op, const uint32_t* din, uint32_t* dout, uint32_t n, uint32_t iw, uint32_t ow, uint32_t param) {
    switch (op) {
#define LANE(OP, IW, OW) case OP: return launch<OP, IW, OW, false>(din, dout, n, iw, ow, param);
#define COOPK(OP, IW, OW) case OP: return launch<OP, IW, OW, true>(din, dout, n, iw, ow, param);
        LANE(OP_FR_MUL, 16, 8) LANE(OP_FR_MUL_WAVE, 16, 8) LANE(OP_FR_SQR, 8, 8) LANE(OP_FR_TO_MONT, 8, 8) LANE(OP_FR_FROM_MONT, 8, 8)
        LANE(OP_FR_ADD, 16, 8) LANE(OP_FR_SUB, 16, 8) LANE(OP_FR_ADD_WAVE, 16, 8) LANE(OP_FR_SUB_WAVE, 16, 8) LANE(OP_FR_ADDSUB_WAVE, 17, 8)
        LANE(OP_FR_NEG, 8, 8) LANE(OP_FR_MUL_CHAIN, 16, 72) LANE(OP_FR_MUL_WAVE_CHAIN, 16, 72)
        LANE(OP_FQ_MUL, 16, 8) LANE(OP_FQ_ADD, 16, 8) LANE(OP_FQ_SUB, 16, 8) LANE(OP_FQ_NEG, 8, 8) LANE(OP_FQ_TO_MONT, 8, 8)
        LANE(OP_FQ_FROM_MONT, 8, 8) LANE(OP_FQ_MUL_CHAIN, 16, 72)
        LANE(OP_FR_INV, 8, 8)
        LANE(OP_DIV_DIGITS, 16, 16) LANE(OP_DIV_SHORT, 16, 16) LANE(OP_DIV_2BY1, 6, 6) LANE(OP_DIV_RECIP, 7, 6) LANE(OP_DIV_3BY2, 10, 8)
        LANE(OP_DIV_128, 16, 16)
        COOPK(OP_COOP4, 16, 8) COOPK(OP_COOP4R, 17, 8) COOPK(OP_ADDSUB_COOP4, 17, 8) COOPK(OP_COOP4_CHAIN, 16, 72)
        COOPK(OP_COOP4_FUSED_CHAIN, 48, 88)
#undef LANE
#undef COOPK
    }
    fprintf(stderr, "unknown op %u\n", op);
    return 2;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::vector<uint32_t> file;
    {
        uint32_t buf[4096];
        size_t got;
        while ((got = fread(buf, 4, 4096, f)) > 0) file.insert(file.end(), buf, buf + got);
        fclose(f);
    }
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    size_t pos = 0;
    int sections = 0;
    while (pos < file.size()) {
        if (file.size() - pos < 5) {
            fprintf(stderr, "truncated section header\n");
            return 2;
        }
        const uint32_t op = file[pos], n = file[pos + 1], iw = file[pos + 2], ow = file[pos + 3], param = file[pos + 4];
        pos += 5;
        const bool coop = op >= OP_COOP4;
        if (n == 0 || n % (coop ? 16u : 64u) != 0 || iw == 0 || ow == 0 || iw > 64 || ow > 128 || n > (1u << 22) || param > 4096 ||
            (size_t)n * iw > file.size() - pos) {
            fprintf(stderr, "bad section (op %u, n %u, %u -> %u words)\n", op, n, iw, ow);
            return 2;
        }
        uint32_t *din = nullptr, *dout = nullptr;
        HIP_OK(hipMalloc(&din, (size_t)n * iw * 4));
        HIP_OK(hipMalloc(&dout, (size_t)n * ow * 4));
        HIP_OK(hipMemcpy(din, file.data() + pos, (size_t)n * iw * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(dout, 0xa5, (size_t)n * ow * 4));
        const int rc = dispatch(op, din, dout, n, iw, ow, param);
        if (rc) return rc;
        std::vector<uint32_t> res((size_t)n * ow);
        HIP_OK(hipMemcpy(res.data(), dout, res.size() * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(din));
        HIP_OK(hipFree(dout));
        if (fwrite(res.data(), 4, res.size(), fo) != res.size()) {
            fprintf(stderr, "short write\n");
            return 2;
        }
        pos += (size_t)n * iw;
        ++sections;
    }
    fclose(fo);
    printf("fr_primitives: %d sections\n", sections);
    return 0;
}
