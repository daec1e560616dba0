// Device harness of tests/test_gpu_point_codec.py (gfx950): runs the primitives of r1cs/point_codec_gfx950.hpp (the roots in Fq and
// Fq2, the order tests, the point codec of both groups) in full 64-lane waves on operand records read from a file, one record per
// lane, and writes the raw result words to a file.  It holds no expected values: the test compares with Python integers.  The
// per-record function, the ops and the record layouts are tests/native/point_codec_ops.hpp; the same file goes through
// point_codec_host.cc on the CPU.
//
//   point_codec IN OUT
//   IN  = sections { u32 op, n, in_words, out_words, param; u32 data[n * in_words] }   (n: records = lanes, a multiple of 64)
//   OUT = the sections' results back to back, (n + 64) * out_words u32 each: 64 guard records follow the results
//
// One kernel instantiation per op, in workgroups of one wave as the library's kernels (codec.hip).
//
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I circom-witnesscalc_amd/r1cs
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "point_codec_ops.hpp"

using namespace codec_ops;

constexpr uint32_t THREADS = 64;

template <uint32_t OP>
__global__ void __launch_bounds__(THREADS) codec_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    run_record<OP>(in + (size_t)t * in_words(OP), out + (size_t)t * out_words(OP));
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
static int launch(const uint32_t* din, uint32_t* dout, uint32_t n) {
    codec_kernel<OP><<<n / THREADS, THREADS>>>(din, dout, n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    return 0;
}

static int dispatch(uint32_t op, const uint32_t* din, uint32_t* dout, uint32_t n) {
    switch (op) {
#define CASE(OP) case OP: return launch<OP>(din, dout, n);
        CASE(OP_FQ_SQRT) CASE(OP_FQ2_SQRT) CASE(OP_FQ_IS_LARGER) CASE(OP_FQ2_IS_LARGER) CASE(OP_G1_ENCODE) CASE(OP_G2_ENCODE) CASE(OP_G1_DECODE)
        CASE(OP_G2_DECODE)
#undef CASE
    }
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
        if (op < OP_FQ_SQRT || op >= OP_END || n == 0 || n % 64u != 0 || n > MAX_RECORDS || iw != in_words(op) || ow != out_words(op) ||
            (size_t)n * iw > file.size() - pos) {
            fprintf(stderr, "bad section (op %u, n %u, %u -> %u words)\n", op, n, iw, ow);
            return 2;
        }
        const size_t out_n = (size_t)(n + GUARD) * ow;
        uint32_t *din = nullptr, *dout = nullptr;
        HIP_OK(hipMalloc(&din, (size_t)n * iw * 4));
        HIP_OK(hipMalloc(&dout, out_n * 4));
        HIP_OK(hipMemcpy(din, file.data() + pos, (size_t)n * iw * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(dout, 0xa5, out_n * 4));
        const int rc = dispatch(op, din, dout, n);
        if (rc) return rc;
        std::vector<uint32_t> res(out_n);
        HIP_OK(hipMemcpy(res.data(), dout, out_n * 4, hipMemcpyDeviceToHost));
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
    printf("point_codec: %d sections\n", sections);
    return 0;
}
