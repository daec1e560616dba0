// Host-side plumbing that the library's .hip files share: the owners of device memory, streams and events (device_owners.hpp,
// with the error text), the launch grid, the workspace carver, the table of squarings that the kernels build powers from, and
// the device side of a key setup with its phase timer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "../csrc/fr_gfx950.hpp"
#include "device_owners.hpp"

namespace cwc_r1cs {

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

// points per piece of a call that sends a long list through the device in pieces: the knob's value when it lies in
// [1, 2^24], else 2^18; read at each call
inline uint64_t piece_points(const char* knob) {
    const char* v = getenv(knob);
    if (!v || !*v) return 1ull << 18;
    const unsigned long long c = strtoull(v, nullptr, 10);
    return c >= 1 && c <= (1ull << 24) ? c : 1ull << 18;
}

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
// derives from the trapdoor and is zeroed before it is released.  The destructor's body does that, and it runs while every
// member is alive; the members then go in reverse order: `secret` (zeroed by now), `work`, the events, and the stream last,
// after the buffers, whose release waits for what was enqueued on it.
template <int N_EVENTS>
struct SetupDevice {
    Stream s;
    PhaseEvents<N_EVENTS> ev;
    DeviceBuf work, secret;
    size_t secret_bytes = 0;
    hipError_t open(size_t secret_size, size_t work_size) {
        secret_bytes = secret_size;
        hipError_t e = s.create();
        if (e == hipSuccess) e = ev.on();
        if (e == hipSuccess) e = secret.alloc(secret_bytes);
        if (e == hipSuccess) e = work.alloc(work_size);
        return e;
    }
    ~SetupDevice() {
        if (secret) {
            (void)hipMemsetAsync(secret.as(), 0, secret_bytes, s);
            (void)hipStreamSynchronize(s);
        }
    }
};

// The N phase times of the last call of a kind in the process, as its *_phase_ms function reports them.
template <int N>
struct PhaseTimes {
    std::mutex mutex;
    float ms[N];
    bool valid = false;
    // phase i lies between events i and i + 1 (all completed); a phase whose bit of `idle` is set enqueued nothing: 0 ms
    void record(const PhaseEvents<N + 1>& ev, uint32_t idle = 0) {
        float t[N];
        const bool ok = ev.elapsed(t) == hipSuccess;
        for (int i = 0; i < N; ++i)
            if ((idle >> i) & 1u) t[i] = 0.0f;
        std::lock_guard<std::mutex> lock(mutex);
        if (ok) memcpy(ms, t, sizeof t);
        valid = ok;
    }
    // times that the caller added up itself (a call that runs in pieces)
    void store(const float (&t)[N], bool ok) {
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
