// The unwinding paths of r1cs/device_owners.hpp, on a machine without a HIP device: there every allocation and every stream or
// event creation fails, so each owner is driven through its failure path and must come out empty, report the error, and be
// safe to move, reset and destroy.  Built by tests/test_device_owners_host.py with -fsanitize=address,undefined against the HIP
// runtime library.  Prints "DEVICE" and does nothing where a device is visible; otherwise one "FAIL ..." line per broken
// expectation, then "OK <checks>" or "FAILED <n>".
#include <stdio.h>

#include "../../circom-witnesscalc_amd/r1cs/device_owners.hpp"

using namespace cwc_r1cs;

static int checks = 0, failures = 0;
#define CHECK(c)                                             \
    do {                                                     \
        ++checks;                                            \
        if (!(c)) {                                          \
            ++failures;                                      \
            printf("FAIL line %d: %s\n", __LINE__, #c);     \
        }                                                    \
    } while (0)

static bool empty(const DeviceBuf& b) { return !b && b.as() == nullptr && b.bytes() == 0 && b.device() == -1; }
static bool empty(const Workspace& w) { return w.bytes() == 0 && w.as() == nullptr; }
static bool empty(const Stream& s) { return (hipStream_t)s == nullptr; }
static bool starts_with(const std::string& s, const char* p) { return s.rfind(p, 0) == 0; }

static void device_buf() {
    DeviceBuf b;
    CHECK(empty(b));
    b.reset();
    CHECK(b.release() == nullptr);
    CHECK(b.alloc(64) != hipSuccess);
    CHECK(empty(b));
    CHECK(b.alloc(0) != hipSuccess);
    CHECK(empty(b));
    const char bytes[16] = {};
    CHECK(b.upload(bytes, sizeof bytes) != hipSuccess);
    CHECK(empty(b));
    DeviceBuf c(std::move(b));
    CHECK(empty(b) && empty(c));
    b = std::move(c);
    CHECK(empty(b) && empty(c));
    DeviceBuf& self = b;
    b = std::move(self);
    CHECK(empty(b));
    c.reset();
    b.reset();
}

static void workspace() {
    Workspace w;
    CHECK(empty(w));
    std::string err;
    CHECK(w.ensure(0, "allocating nothing", err) && err.empty());  // nothing to grow to
    CHECK(empty(w));
    CHECK(!w.ensure(1024, "allocating the test workspace", err));
    CHECK(starts_with(err, "r1cs: allocating the test workspace: ") && err.size() > 37);
    CHECK(empty(w));
    CHECK(!w.ensure(16, "allocating the test workspace", err));  // a failed grow recorded no size: the next call tries again
    CHECK(empty(w));
    Workspace v(std::move(w));
    CHECK(empty(v) && empty(w));
    w = std::move(v);
    CHECK(empty(v) && empty(w));
}

static void stream() {
    Stream s;
    CHECK(empty(s));
    CHECK(s.create() != hipSuccess);
    CHECK(empty(s));
    Stream t(std::move(s));
    CHECK(empty(s) && empty(t));
    s = std::move(t);
    CHECK(empty(s) && empty(t));
    s.reset();
}

static void phase_events() {
    PhaseEvents<5> ev;
    float ms[4] = {-1, -1, -1, -1};
    CHECK(!ev.enabled());
    CHECK(ev.elapsed(ms) != hipSuccess && ms[0] == -1);
    ev.record(0, nullptr);  // off: records nothing
    CHECK(ev.on() != hipSuccess);
    CHECK(!ev.enabled());
    CHECK(ev.on() != hipSuccess);  // twice in a row
    CHECK(!ev.enabled());
    ev.off();
    ev.off();
    PhaseEvents<5> other(std::move(ev));
    CHECK(!ev.enabled() && !other.enabled());
    ev = std::move(other);
    CHECK(!ev.enabled() && !other.enabled());
    CHECK(ev.elapsed(ms) != hipSuccess);
}

static void pinned_stage() {
    PinnedStage p;
    CHECK(p.bytes() == 0);
    const char src[64] = {};
    char dst[64];
    CHECK(p.send(dst, src, sizeof src, nullptr) != hipSuccess);
    CHECK(p.bytes() == 0);
    CHECK(p.send(dst, src, sizeof src, nullptr) != hipSuccess);  // and again, from whatever the first attempt left
    CHECK(p.bytes() == 0);
    PinnedStage q(std::move(p));
    CHECK(p.bytes() == 0 && q.bytes() == 0);
    p = std::move(q);
    CHECK(p.bytes() == 0 && q.bytes() == 0);
    p.reset();
    p.reset();
}

static void staged_run() {
    const char in[32] = {};
    char out[32] = {1};
    int calls = 0;
    std::string err;
    const bool ok = run_staged({sizeof in, sizeof out}, {{in, sizeof in, 0, 0}}, {{out, sizeof out, 1, 0}}, "staging the test rows", "running the test",
                               [&](unsigned char* const*, hipStream_t, std::string&) {
                                   ++calls;
                                   return true;
                               },
                               err);
    CHECK(!ok);
    CHECK(calls == 0);  // nothing is enqueued when staging failed
    CHECK(starts_with(err, "r1cs: staging the test rows: "));
    CHECK(out[0] == 1);
}

int main() {
    int n = 0;
    if (hipGetDeviceCount(&n) == hipSuccess && n > 0) {
        puts("DEVICE");
        return 0;
    }
    CHECK(starts_with(hip_err("doing this", hipErrorOutOfMemory), "r1cs: doing this: "));
    device_buf();
    workspace();
    stream();
    phase_events();
    pinned_stage();
    staged_run();
    if (failures) {
        printf("FAILED %d\n", failures);
        return 1;
    }
    printf("OK %d\n", checks);
    return 0;
}
