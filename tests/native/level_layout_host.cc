// Host-only check of the thread decode that the all-level stage kernels share (r1cs/ptau_internal.hpp's level_butterfly, used by
// setup_ptau.hip's idft_levels_stage_kernel and contribute.hip's fr_levels_stage_kernel): built with -fsanitize=address,undefined
// by tests/test_level_layout_host.py, no HIP and no device.  For every top in 1 .. 16 and every stage s < top it decodes all
// v < 2^top and checks
//   partition    s < m <= top, grp < 2^(m-s-1), k < 2^s; the two slots of every butterfly, lo = 2^m - 1 + grp 2^(s+1) + k and
//                lo + 2^s, are taken once each, and together they are every slot of the levels s + 1 .. top and no other;
//                the idle v are those with w = 0, w being v mod 2^(top-s) while top - s >= 6 and v >> s in the last five stages
//   one k        top - s >= 6: the active lanes of every wave of 64 consecutive v have one k
//   next k       top - s < 6: a v with k < 2^s - 1 is followed by the same (m, grp) with k + 1
//   bounds       lo + 2^s < 2^(m+1) - 1, and k << tw_shift < N / 2 for tw_shift = log2(N) - 1 - s, N = 2^top and N = 2^(top+1)
// A violation prints a line "FAIL ..." (ten per stage at the most) and makes the exit code 1.  Every stage prints one line
//   top s layout active idle max_k max_m waves
// (layout: "wave" or "lane"; waves: the waves whose k was compared), which the Python test holds against the closed forms.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../circom-witnesscalc_amd/r1cs/ptau_internal.hpp"

namespace {

int g_failures = 0, g_stage_failures = 0;

#define FAIL(...)                       \
    do {                                \
        ++g_failures;                   \
        if (++g_stage_failures <= 10) { \
            printf("FAIL ");            \
            printf(__VA_ARGS__);        \
            printf("\n");               \
        }                               \
    } while (0)

void stage(uint32_t top, uint32_t s) {
    g_stage_failures = 0;
    const uint32_t span = top - s, half = 1u << s;
    const bool by_k = span >= 6;
    const uint64_t threads = 1ull << top, slots = (2ull << top) - 1;
    std::vector<uint8_t> taken(slots, 0);
    std::vector<uint8_t> active(threads, 0);
    std::vector<cwc_ptau::LevelButterfly> dec(threads);
    uint64_t n_active = 0, n_idle = 0, waves = 0;
    uint32_t max_k = 0, max_m = 0;
    for (uint64_t v = 0; v < threads; ++v) {
        cwc_ptau::LevelButterfly b{~0u, ~0u, ~0u};
        const bool on = cwc_ptau::level_butterfly((uint32_t)v, top, s, b);
        const uint64_t w = by_k ? v & ((1ull << span) - 1) : v >> s;  // the layout as the header states it
        if (on != (w != 0)) FAIL("top %u s %u v %llu: active %d, w %llu", top, s, (unsigned long long)v, (int)on, (unsigned long long)w);
        if (!on) {
            ++n_idle;
            continue;
        }
        ++n_active;
        if (!(b.m > s && b.m <= top) || b.k >= half || (uint64_t)b.grp >= (1ull << (b.m - s - 1))) {
            FAIL("top %u s %u v %llu: (m, grp, k) = (%u, %u, %u) out of range", top, s, (unsigned long long)v, b.m, b.grp, b.k);
            continue;  // its slots are not looked up
        }
        active[v] = 1;
        dec[v] = b;
        if (b.k > max_k) max_k = b.k;
        if (b.m > max_m) max_m = b.m;
        const uint64_t lo = ((1ull << b.m) - 1) + ((uint64_t)b.grp << (s + 1)) + b.k, hi = lo + half;
        if (hi >= (2ull << b.m) - 1) {
            FAIL("top %u s %u v %llu: slot %llu is past level %u", top, s, (unsigned long long)v, (unsigned long long)hi, b.m);
            continue;
        }
        if (taken[lo]++ || taken[hi]++) FAIL("top %u s %u v %llu: a slot of (%u, %u, %u) is taken twice", top, s, (unsigned long long)v, b.m, b.grp, b.k);
        for (uint32_t log_n = top; log_n <= top + 1; ++log_n) {
            const uint32_t tw_shift = log_n - 1 - s;
            if (((uint64_t)b.k << tw_shift) >= (1ull << (log_n - 1)))
                FAIL("top %u s %u v %llu: twiddle index %llu for N = 2^%u", top, s, (unsigned long long)v, (unsigned long long)((uint64_t)b.k << tw_shift), log_n);
        }
    }
    for (uint64_t i = 0; i < slots; ++i) {
        const bool wanted = i + 1 >= (2ull << s);  // the levels s + 1 .. top begin at the slot 2^(s+1) - 1
        if ((taken[i] == 1) != wanted) FAIL("top %u s %u: slot %llu is taken %u times", top, s, (unsigned long long)i, (unsigned)taken[i]);
    }
    if (by_k) {
        for (uint64_t base = 0; base < threads; base += 64, ++waves) {
            bool have = false;
            uint32_t k = 0;
            for (uint64_t v = base; v < base + 64; ++v) {
                if (!active[v]) continue;
                if (have && dec[v].k != k) FAIL("top %u s %u: the wave at v %llu has the k %u and %u", top, s, (unsigned long long)base, k, dec[v].k);
                k = dec[v].k;
                have = true;
            }
            if (!have) FAIL("top %u s %u: the wave at v %llu is idle", top, s, (unsigned long long)base);
        }
    } else {
        for (uint64_t v = 0; v < threads; ++v) {
            if (!active[v] || dec[v].k + 1 >= half) continue;
            const bool next = v + 1 < threads && active[v + 1] && dec[v + 1].m == dec[v].m && dec[v + 1].grp == dec[v].grp && dec[v + 1].k == dec[v].k + 1;
            if (!next) FAIL("top %u s %u v %llu: the next thread does not have k + 1 of the same group", top, s, (unsigned long long)v);
        }
    }
    printf("%u %u %s %llu %llu %u %u %llu\n", top, s, by_k ? "wave" : "lane", (unsigned long long)n_active, (unsigned long long)n_idle, max_k, max_m,
           (unsigned long long)waves);
}

}  // namespace

int main() {
    for (uint32_t top = 1; top <= 16; ++top)
        for (uint32_t s = 0; s < top; ++s) stage(top, s);
    printf("failures %d\n", g_failures);
    return g_failures ? 1 : 0;
}
