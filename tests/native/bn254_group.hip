// Device harness of tests/test_gpu_bn254_group.py (gfx950): runs the G1 / G2 group law of r1cs/fq_gfx950.hpp (xyzz_add,
// xyzz_add_affine, xyzz_dbl, xyzz_neg, xyzz_to_affine, xyzz_mul, xyzz_mul_short) in full 64-lane waves on operand records read from
// a file, one record per lane, and writes the raw result limbs to a file.  It holds no expected values: the test compares with
// Python integers.  The record-file format is that of fr_primitives.hip.
//
//   bn254_group IN OUT
//   IN  = sections { u32 op, n, in_words, out_words, param; u32 data[n * in_words] }   (n: records = lanes, a multiple of 64;
//         param: 1 = G1, 2 = G2)
//   OUT = the sections' results back to back, n * out_words u32 each
//
// A coordinate is E = 8 words (G1, Fq) or 16 words (G2, Fq2: c0, c1), Montgomery form; XYZZ = 4 E (X, Y, ZZ, ZZZ), affine = 2 E.
//   add:        p XYZZ, q XYZZ   -> p + q XYZZ, then its affine form        mul, mul_short:  p XYZZ, k (8 words) -> k p XYZZ
//   add_affine: p XYZZ, q affine -> p + q XYZZ, then its affine form        dbl: p -> 2 p XYZZ, then its affine form
//   neg:        p -> -p XYZZ                                                to_affine: p -> affine
//
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I circom-witnesscalc_amd/r1cs
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "fq_gfx950.hpp"

using namespace cwc_g16;

enum Op : uint32_t { OP_ADD = 1, OP_ADD_AFFINE, OP_DBL, OP_NEG, OP_TO_AFFINE, OP_MUL, OP_MUL_SHORT };

__device__ __forceinline__ Fq ld8(const uint32_t* p) {
    Fq x;
#pragma unroll
    for (int i = 0; i < 8; ++i) x.v[i] = p[i];
    return x;
}
__device__ __forceinline__ void st8(uint32_t* p, const Fq& x) {
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = x.v[i];
}

template <class T>
struct IO;
template <>
struct IO<FqT> {
    static constexpr uint32_t W = 8;
    static __device__ __forceinline__ Fq ld(const uint32_t* p) { return ld8(p); }
    static __device__ __forceinline__ void st(uint32_t* p, const Fq& x) { st8(p, x); }
};
template <>
struct IO<Fq2T> {
    static constexpr uint32_t W = 16;
    static __device__ __forceinline__ Fq2 ld(const uint32_t* p) { return Fq2{ld8(p), ld8(p + 8)}; }
    static __device__ __forceinline__ void st(uint32_t* p, const Fq2& x) {
        st8(p, x.c0);
        st8(p + 8, x.c1);
    }
};

template <class T>
__device__ __forceinline__ Xyzz<T> ld_xyzz(const uint32_t* p) {
    constexpr uint32_t W = IO<T>::W;
    return Xyzz<T>{IO<T>::ld(p), IO<T>::ld(p + W), IO<T>::ld(p + 2 * W), IO<T>::ld(p + 3 * W)};
}
template <class T>
__device__ __forceinline__ void st_xyzz(uint32_t* p, const Xyzz<T>& x) {
    constexpr uint32_t W = IO<T>::W;
    IO<T>::st(p, x.X);
    IO<T>::st(p + W, x.Y);
    IO<T>::st(p + 2 * W, x.ZZ);
    IO<T>::st(p + 3 * W, x.ZZZ);
}
template <class T>
__device__ __forceinline__ void st_affine(uint32_t* p, const Affine<T>& a) {
    IO<T>::st(p, a.x);
    IO<T>::st(p + IO<T>::W, a.y);
}

// words per record, in and out, of an op over coordinates of W words
__host__ __device__ constexpr uint32_t in_words(uint32_t op, uint32_t W) {
    return op == OP_ADD ? 8 * W : op == OP_ADD_AFFINE ? 6 * W : op == OP_MUL || op == OP_MUL_SHORT ? 4 * W + 8 : 4 * W;
}
__host__ __device__ constexpr uint32_t out_words(uint32_t op, uint32_t W) {
    return op == OP_ADD || op == OP_ADD_AFFINE || op == OP_DBL ? 6 * W : op == OP_TO_AFFINE ? 2 * W : 4 * W;
}

// one record per lane; n is a multiple of 64, so every wave is full or absent; four waves per workgroup
template <class T, uint32_t OP>
__global__ void __launch_bounds__(256) group_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    constexpr uint32_t W = IO<T>::W, IW = in_words(OP, W), OW = out_words(OP, W);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t* r = in + (size_t)t * IW;
    uint32_t* o = out + (size_t)t * OW;
    const Xyzz<T> p = ld_xyzz<T>(r);
    if constexpr (OP == OP_ADD || OP == OP_ADD_AFFINE || OP == OP_DBL) {
        Xyzz<T> s;
        if constexpr (OP == OP_ADD) s = xyzz_add(p, ld_xyzz<T>(r + 4 * W));
        if constexpr (OP == OP_ADD_AFFINE) s = xyzz_add_affine(p, Affine<T>{IO<T>::ld(r + 4 * W), IO<T>::ld(r + 5 * W)});
        if constexpr (OP == OP_DBL) s = xyzz_dbl(p);
        st_xyzz<T>(o, s);
        st_affine<T>(o + 4 * W, xyzz_to_affine(s));
    }
    if constexpr (OP == OP_NEG) st_xyzz<T>(o, xyzz_neg(p));
    if constexpr (OP == OP_TO_AFFINE) st_affine<T>(o, xyzz_to_affine(p));
    if constexpr (OP == OP_MUL) st_xyzz<T>(o, xyzz_mul(p, ld8(r + 4 * W)));
    if constexpr (OP == OP_MUL_SHORT) st_xyzz<T>(o, xyzz_mul_short(p, ld8(r + 4 * W)));
}

#define HIP_OK(x)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                        \
            return 3;                                                                      \
        }                                                                                  \
    } while (0)

template <class T, uint32_t OP>
static int launch(const uint32_t* din, uint32_t* dout, uint32_t n, uint32_t iw, uint32_t ow) {
    constexpr uint32_t W = IO<T>::W;
    if (iw != in_words(OP, W) || ow != out_words(OP, W)) {
        fprintf(stderr, "op %u: record of %u -> %u words, expected %u -> %u\n", OP, iw, ow, in_words(OP, W), out_words(OP, W));
        return 2;
    }
    const uint32_t block = 256;
    group_kernel<T, OP><<<(n + block - 1) / block, block>>>(din, dout, n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    return 0;
}

template <class T>
static int dispatch(uint32_t op, const uint32_t* din, uint32_t* dout, uint32_t n, uint32_t iw, uint32_t ow) {
    switch (op) {
#define CASE(OP) case OP: return launch<T, OP>(din, dout, n, iw, ow);
        CASE(OP_ADD) CASE(OP_ADD_AFFINE) CASE(OP_DBL) CASE(OP_NEG) CASE(OP_TO_AFFINE) CASE(OP_MUL) CASE(OP_MUL_SHORT)
#undef CASE
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
        const uint32_t op = file[pos], n = file[pos + 1], iw = file[pos + 2], ow = file[pos + 3], group = file[pos + 4];
        pos += 5;
        if (n == 0 || n % 64u != 0 || iw == 0 || ow == 0 || iw > 256 || ow > 256 || n > (1u << 20) || (group != 1 && group != 2) ||
            (size_t)n * iw > file.size() - pos) {
            fprintf(stderr, "bad section (op %u, n %u, %u -> %u words, group %u)\n", op, n, iw, ow, group);
            return 2;
        }
        uint32_t *din = nullptr, *dout = nullptr;
        HIP_OK(hipMalloc(&din, (size_t)n * iw * 4));
        HIP_OK(hipMalloc(&dout, (size_t)n * ow * 4));
        HIP_OK(hipMemcpy(din, file.data() + pos, (size_t)n * iw * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(dout, 0xa5, (size_t)n * ow * 4));
        const int rc = group == 1 ? dispatch<FqT>(op, din, dout, n, iw, ow) : dispatch<Fq2T>(op, din, dout, n, iw, ow);
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
    printf("bn254_group: %d sections\n", sections);
    return 0;
}
