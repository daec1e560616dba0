// Device harness of tests/test_gpu_fq12_tower.py (gfx950): runs the primitives of r1cs/fq12_gfx950.hpp (the Fq2 / Fq6 / Fq12
// tower, the final exponentiation's two parts, the Miller loop's G2 steps) in full 64-lane waves on operand records read from a
// file, one record per lane, and writes the raw result limbs to a file.  It holds no expected values: the test compares with
// Python integers.  The per-record function, the ops and the record layouts are tests/native/fq12_tower_ops.hpp; the same file
// goes through fq12_tower_host.cc on the CPU.
//
//   fq12_tower IN OUT
//   IN  = sections { u32 op, n, in_words, out_words, param; u32 data[n * in_words] }   (n: records = lanes, a multiple of 64)
//   OUT = the sections' results back to back, (n + 64) * out_words u32 each: 64 guard records follow the results
//
// One kernel instantiation per op, in workgroups of one wave as the verifier's kernels (verify.hip), so that every primitive is
// compiled with one call site.  The final exponentiation's slots are a global buffer, SLOT_WORDS per record.
//
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I circom-witnesscalc_amd/r1cs [-DTOWER_FAMILY=f]
// With TOWER_FAMILY = 1 (Fq, Fq2), 2 (Fq6), 3 (Fq12), 4 (cyclotomic squaring and the final exponentiation) or 5 (G2 steps) only
// that family's kernels are built, so that the five programs compile side by side; without it, all of them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "fq12_tower_ops.hpp"

using namespace tower_ops;

#ifndef TOWER_FAMILY
#define TOWER_FAMILY 0
#endif
#define FAMILY(f) (TOWER_FAMILY == 0 || TOWER_FAMILY == (f))

constexpr uint32_t THREADS = 64;

__constant__ FxProg c_fx = fx_prog();

template <uint32_t OP>
__global__ void __launch_bounds__(THREADS) tower_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n,
                                                        uint32_t* __restrict__ slots) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    run_record<OP>(in + (size_t)t * in_words(OP), out + (size_t)t * out_words(OP), c_fx, slots + (size_t)t * SLOT_WORDS);
}

#define HIP_OK(x)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                        \
            return 3;                                                                      \
        }                                                                                  \
    } while (0)

template <uint32_t OP>
static int launch(const uint32_t* din, uint32_t* dout, uint32_t n, uint32_t* slots) {
    tower_kernel<OP><<<n / THREADS, THREADS>>>(din, dout, n, slots);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    return 0;
}

static int dispatch(uint32_t op, const uint32_t* din, uint32_t* dout, uint32_t n, uint32_t* slots) {
    switch (op) {
#define CASE(OP) case OP: return launch<OP>(din, dout, n, slots);
#if FAMILY(1)
        CASE(OP_FQ_HALF) CASE(OP_FQ2_HALF) CASE(OP_FQ2_MUL) CASE(OP_FQ2_SQR) CASE(OP_FQ2_INV) CASE(OP_FQ2_CONJ) CASE(OP_FQ2_MUL_FQ)
        CASE(OP_FQ2_MUL_XI)
#endif
#if FAMILY(2)
        CASE(OP_FQ6_MUL) CASE(OP_FQ6_MUL_01) CASE(OP_FQ6_MUL_FQ2) CASE(OP_FQ6_MUL_V) CASE(OP_FQ6_INV)
#endif
#if FAMILY(3)
        CASE(OP_FQ12_MUL) CASE(OP_FQ12_SQR) CASE(OP_FQ12_INV) CASE(OP_FQ12_CONJ) CASE(OP_FQ12_MUL_LINE) CASE(OP_FQ12_MUL_LINE_AT)
        CASE(OP_FQ12_FROB)
#endif
#if FAMILY(4)
        CASE(OP_FQ12_CSQ) CASE(OP_FINAL_EASY) CASE(OP_FINAL_HARD)
#endif
#if FAMILY(5)
        CASE(OP_G2_DBL_STEP) CASE(OP_G2_ADD_STEP) CASE(OP_G2_FROB1) CASE(OP_G2_NEG_FROB2) CASE(OP_MILLER_STEP)
#endif
#undef CASE
    }
    fprintf(stderr, "op %u is not in this build (TOWER_FAMILY %d)\n", op, TOWER_FAMILY);
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
        const uint32_t op = file[pos], n = file[pos + 1], iw = file[pos + 2], ow = file[pos + 3];
        pos += 5;
        if (op < OP_FQ_HALF || op >= OP_END || n == 0 || n % 64u != 0 || n > MAX_RECORDS || iw != in_words(op) || ow != out_words(op) ||
            (size_t)n * iw > file.size() - pos) {
            fprintf(stderr, "bad section (op %u, n %u, %u -> %u words)\n", op, n, iw, ow);
            return 2;
        }
        const size_t out_n = (size_t)(n + GUARD) * ow;
        uint32_t *din = nullptr, *dout = nullptr, *slots = nullptr;
        HIP_OK(hipMalloc(&din, (size_t)n * iw * 4));
        HIP_OK(hipMalloc(&dout, out_n * 4));
        HIP_OK(hipMemcpy(din, file.data() + pos, (size_t)n * iw * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(dout, 0xa5, out_n * 4));
        if (op == OP_FINAL_HARD) {
            HIP_OK(hipMalloc(&slots, (size_t)n * SLOT_WORDS * 4));
            HIP_OK(hipMemset(slots, 0xa5, (size_t)n * SLOT_WORDS * 4));
        }
        const int rc = dispatch(op, din, dout, n, slots);
        if (rc) return rc;
        std::vector<uint32_t> res(out_n);
        HIP_OK(hipMemcpy(res.data(), dout, out_n * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(din));
        HIP_OK(hipFree(dout));
        if (slots) HIP_OK(hipFree(slots));
        if (fwrite(res.data(), 4, res.size(), fo) != res.size()) {
            fprintf(stderr, "short write\n");
            return 2;
        }
        pos += (size_t)n * iw;
        ++sections;
    }
    fclose(fo);
    printf("fq12_tower: %d sections\n", sections);
    return 0;
}
