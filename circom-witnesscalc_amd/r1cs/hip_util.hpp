// Host-side plumbing that the library's .hip files share: the error text, the launch grid, the workspace carver, the table of
// squarings that the kernels build powers from, and the device side of a key setup with its phase timer.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "../csrc/fr_gfx950.hpp"

namespace cwc_r1cs {

std::string hip_err(const char* what, hipError_t e);  // check.hip: "r1cs: <what>: <the runtime's text>"

// blocks of `block` threads for n threads, at least one
inline uint32_t blocks_for(uint64_t n, uint32_t block) { return (uint32_t)std::max<uint64_t>(1, (n + block - 1) / block); }

// offsets into one allocation, every piece 256-byte aligned
struct Carve {
    size_t o = 0;
    size_t take(size_t bytes) {
        const size_t at = o;
        o += (bytes + 255) & ~(size_t)255;
        return at;
    }
};

constexpr uint32_t MAX_DOMAIN_POWER = 27;  // 2-adicity of r is 28; the coset needs a 2n-th root

struct Pows {
    cwc::Fr v[MAX_DOMAIN_POWER + 1];  // base^(2^b), Montgomery form
};
inline Pows powers_of(const cwc::Fr& base) {  // Montgomery form
    Pows p;
    p.v[0] = base;
    for (uint32_t b = 1; b <= MAX_DOMAIN_POWER; ++b) p.v[b] = cwc::fr_mul(p.v[b - 1], p.v[b - 1]);
    return p;
}

// The device side of one setup call: a stream, N_EVENTS events around its phases, the workspace, and `secret`, which holds what
// derives from the trapdoor and is zeroed before it is released.
template <int N_EVENTS>
struct SetupDevice {
    hipStream_t s = nullptr;
    void *secret = nullptr, *work = nullptr;
    size_t secret_bytes = 0;
    hipEvent_t ev[N_EVENTS] = {};
    hipError_t open(size_t secret_size, size_t work_size) {
        secret_bytes = secret_size;
        hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        for (hipEvent_t& v : ev)
            if (e == hipSuccess) e = hipEventCreate(&v);
        if (e == hipSuccess) e = hipMalloc(&secret, secret_bytes);
        if (e == hipSuccess) e = hipMalloc(&work, work_size);
        return e;
    }
    ~SetupDevice() {
        if (secret) {
            (void)hipMemsetAsync(secret, 0, secret_bytes, s);
            (void)hipStreamSynchronize(s);
            (void)hipFree(secret);
        }
        if (work) (void)hipFree(work);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (s) (void)hipStreamDestroy(s);
    }
};

// The N phase times of the last call of a kind in the process, as its *_phase_ms function reports them.
template <int N>
struct PhaseTimes {
    std::mutex mutex;
    float ms[N];
    bool valid = false;
    // phase i lies between ev[i] and ev[i + 1] (all completed); a phase whose bit of `idle` is set enqueued nothing: 0 ms
    void record(const hipEvent_t* ev, uint32_t idle = 0) {
        float t[N];
        bool ok = true;
        for (int i = 0; i < N; ++i) {
            ok = ok && hipEventElapsedTime(t + i, ev[i], ev[i + 1]) == hipSuccess;
            if ((idle >> i) & 1u) t[i] = 0.0f;
        }
        std::lock_guard<std::mutex> lock(mutex);
        if (ok) memcpy(ms, t, sizeof t);
        valid = ok;
    }
    int read(float* out) {  // 0, or 1 when there is nothing to report
        if (!out) return 1;
        std::lock_guard<std::mutex> lock(mutex);
        if (!valid) return 1;
        memcpy(out, ms, sizeof ms);
        return 0;
    }
};

}  // namespace cwc_r1cs
