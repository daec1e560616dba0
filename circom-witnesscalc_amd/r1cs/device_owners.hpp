// Who owns what on the device: the one place in r1cs/ that allocates and frees device memory, pinned host memory, streams and
// events.  Every owner is move-only, empty when default-constructed and safe to destroy empty; a failed call leaves it empty
// and returns the runtime's error; assigning to one releases what it held and leaves the source empty.  The handle structs hold these (r1cs_internal.hpp, groth16_internal.hpp), so this header
// needs no more of HIP than the runtime's C API and compiles with the host compiler.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <string.h>

#include <initializer_list>
#include <string>
#include <utility>

namespace cwc_r1cs {

inline std::string hip_err(const char* what, hipError_t e) { return std::string("r1cs: ") + what + ": " + hipGetErrorString(e); }

// One hipMalloc allocation, its size and the device it was made on.  It is freed with that device current, whichever device
// the caller is on, and the caller's device is restored.
class DeviceBuf {
    void* p_ = nullptr;
    size_t bytes_ = 0;
    int device_ = -1;

public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)), device_(std::exchange(o.device_, -1)) {}
    DeviceBuf& operator=(DeviceBuf o) noexcept {  // (o took the source's, and takes what was held here with it)
        std::swap(p_, o.p_);
        std::swap(bytes_, o.bytes_);
        std::swap(device_, o.device_);
        return *this;
    }
    ~DeviceBuf() { reset(); }

    // on the current device, after releasing what was held; an empty array still gets an address (4 bytes)
    hipError_t alloc(size_t bytes) {
        reset();
        hipError_t e = hipGetDevice(&device_);
        if (e == hipSuccess) e = hipMalloc(&p_, bytes < 4 ? 4 : bytes);
        if (e == hipSuccess)
            bytes_ = bytes;
        else
            release();
        return e;
    }
    // allocates `bytes` and copies them from `src` (synchronous)
    hipError_t upload(const void* src, size_t bytes) {
        hipError_t e = alloc(bytes);
        if (e == hipSuccess && bytes) e = hipMemcpy(p_, src, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) reset();
        return e;
    }
    void reset() {
        if (!p_) return;
        int cur = -1;
        const bool elsewhere = hipGetDevice(&cur) == hipSuccess && cur != device_;
        if (elsewhere) (void)hipSetDevice(device_);
        (void)hipFree(release());
        if (elsewhere) (void)hipSetDevice(cur);
    }
    void* release() {  // the allocation outlives the owner: the caller's to free, or to keep until the process ends
        bytes_ = 0;
        device_ = -1;
        return std::exchange(p_, nullptr);
    }
    template <class T = void>
    T* as() const { return static_cast<T*>(p_); }
    size_t bytes() const { return bytes_; }
    int device() const { return device_; }
    explicit operator bool() const { return p_ != nullptr; }
};

// A workspace that only grows: calls that need no more than it holds reuse it.
class Workspace {
    DeviceBuf buf_;

public:
    // at least `bytes`; `what` names the allocation in the error ("allocating the ... workspace")
    bool ensure(size_t bytes, const char* what, std::string& err) {
        if (buf_.bytes() >= bytes) return true;
        buf_.reset();  // (synchronises with earlier work that used it)
        const hipError_t e = buf_.alloc(bytes);
        if (e != hipSuccess) err = hip_err(what, e);
        return e == hipSuccess;
    }
    size_t bytes() const { return buf_.bytes(); }
    template <class T = void>
    T* as() const { return buf_.as<T>(); }
};

// A non-blocking stream.
class Stream {
    hipStream_t s_ = nullptr;

public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    Stream& operator=(Stream o) noexcept {
        std::swap(s_, o.s_);
        return *this;
    }
    ~Stream() { reset(); }
    hipError_t create() {
        reset();
        const hipError_t e = hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
        if (e != hipSuccess) s_ = nullptr;
        return e;
    }
    void reset() {
        if (s_) (void)hipStreamDestroy(s_);
        s_ = nullptr;
    }
    operator hipStream_t() const { return s_; }
};

// N events around the N - 1 phases of a call; all of them exist (timing is on) or none does.
template <int N>
class PhaseEvents {
    hipEvent_t ev_[N] = {};

public:
    PhaseEvents() = default;
    PhaseEvents(PhaseEvents&& o) noexcept { std::swap(ev_, o.ev_); }
    PhaseEvents& operator=(PhaseEvents o) noexcept {
        std::swap(ev_, o.ev_);
        return *this;
    }
    ~PhaseEvents() { off(); }
    hipError_t on() {  // fresh events; off again if one cannot be made
        off();
        for (hipEvent_t& e : ev_) {
            const hipError_t err = hipEventCreate(&e);
            if (err != hipSuccess) {
                e = nullptr;
                off();
                return err;
            }
        }
        return hipSuccess;
    }
    void off() {
        for (hipEvent_t& e : ev_) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }
    bool enabled() const { return ev_[0] != nullptr; }
    void record(int i, hipStream_t s) const {  // nothing while timing is off
        if (enabled()) (void)hipEventRecord(ev_[i], s);
    }
    // waits for the last event; ms[i] is the time between events i and i + 1
    hipError_t elapsed(float (&ms)[N - 1]) const {
        if (!enabled()) return hipErrorNotReady;
        hipError_t e = hipEventSynchronize(ev_[N - 1]);
        for (int i = 0; i < N - 1 && e == hipSuccess; ++i) e = hipEventElapsedTime(ms + i, ev_[i], ev_[i + 1]);
        return e;
    }
};

// Pinned host memory that values pass through on their way to the device, and the event after the last copy out of it.
class PinnedStage {
    void* p_ = nullptr;
    size_t bytes_ = 0;
    hipEvent_t done_ = nullptr;

public:
    PinnedStage() = default;
    PinnedStage(PinnedStage&& o) noexcept
        : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)), done_(std::exchange(o.done_, nullptr)) {}
    PinnedStage& operator=(PinnedStage o) noexcept {
        std::swap(p_, o.p_);
        std::swap(bytes_, o.bytes_);
        std::swap(done_, o.done_);
        return *this;
    }
    ~PinnedStage() { reset(); }
    // `bytes` at src -> d_dst on s: waits for the previous copy out of the buffer, grows the buffer if it is too small,
    // fills it and enqueues the copy
    hipError_t send(void* d_dst, const void* src, size_t bytes, hipStream_t s) {
        hipError_t e = done_ ? hipEventSynchronize(done_) : hipEventCreateWithFlags(&done_, hipEventDisableTiming);
        if (e == hipSuccess && bytes_ < bytes) {
            if (p_) (void)hipHostFree(p_);
            p_ = nullptr;
            bytes_ = 0;
            e = hipHostMalloc(&p_, bytes, hipHostMallocDefault);
            if (e == hipSuccess) bytes_ = bytes;
        }
        if (e == hipSuccess) {
            memcpy(p_, src, bytes);
            e = hipMemcpyAsync(d_dst, p_, bytes, hipMemcpyHostToDevice, s);
        }
        if (e == hipSuccess) e = hipEventRecord(done_, s);
        return e;
    }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        if (done_) (void)hipEventDestroy(done_);
        p_ = nullptr;
        bytes_ = 0;
        done_ = nullptr;
    }
    size_t bytes() const { return bytes_; }
};

// A host range and where it lies on the device: `bytes` at offset `off` of allocation `buf`.
template <class P>
struct HostRange {
    P host;
    size_t bytes;
    int buf;
    size_t off;
};
using HostIn = HostRange<const void*>;
using HostOut = HostRange<void*>;

// The synchronous host entry points: a stream and the allocations of `allocs` bytes are made, the ranges of `in` copied to
// them ("<staging>" names a failure up to here), `enqueue(d, stream, err)` runs with the allocations' addresses d[], the
// ranges of `out` are copied back and the stream is waited for ("<running>"); everything is released on every path.
template <class F>
bool run_staged(std::initializer_list<size_t> allocs, std::initializer_list<HostIn> in, std::initializer_list<HostOut> out,
                const char* staging, const char* running, F&& enqueue, std::string& err) {
    constexpr size_t MAX_ALLOCS = 4;
    Stream s;  // (released last: after the buffers, whose release waits for the work on it)
    DeviceBuf bufs[MAX_ALLOCS];
    unsigned char* d[MAX_ALLOCS] = {};
    hipError_t e = allocs.size() <= MAX_ALLOCS ? s.create() : hipErrorInvalidValue;
    size_t k = 0;
    for (const size_t bytes : allocs) {
        if (e == hipSuccess) e = bufs[k].alloc(bytes);
        d[k] = bufs[k].as<unsigned char>();
        ++k;
    }
    for (const HostIn& i : in)
        if (e == hipSuccess && i.bytes) e = hipMemcpyAsync(d[i.buf] + i.off, i.host, i.bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
        err = hip_err(staging, e);
        return false;
    }
    if (!enqueue(d, (hipStream_t)s, err)) return false;
    for (const HostOut& o : out)
        if (e == hipSuccess && o.bytes) e = hipMemcpyAsync(o.host, d[o.buf] + o.off, o.bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        err = hip_err(running, e);
        return false;
    }
    return true;
}

}  // namespace cwc_r1cs
