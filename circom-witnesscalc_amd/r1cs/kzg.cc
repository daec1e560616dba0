// KZG commitments over a `.ptau` file, host side (include/graph_witness_kzg.h has the definitions): the handle (the file's checks,
// the SRS prefix on the device in canonical form, the Lagrange levels on first use), the sub-batching under the prover's
// workspace cap, the phase events and the C ABI.  The kernels are kzg.hip's (kzg_internal.hpp); a commitment or a witness is one
// gwb_bn254_g1_lincomb_device call per polynomial over the handle's points (contribute.hip, unchanged), the pairings of a check
// one gwb_bn254_pairing_batch_device call per sub-batch (verify.hip).  A folded opening (open_fold_device, verify_fold_device) is
// the same machinery on the fold of a group's polynomials or points, sub-batched over groups, with phase events of its own.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/graph_witness_batch.h"
#include "../../include/graph_witness_groth16_ptau.h"
#include "../../include/graph_witness_groth16_verify.h"
#include "../../include/graph_witness_kzg.h"
#include "bn254_points_gfx950.hpp"
#include "contribute_internal.hpp"
#include "device_owners.hpp"
#include "groth16_internal.hpp"
#include "hip_util.hpp"
#include "kzg_internal.hpp"
#include "ptau_internal.hpp"

using namespace cwc_r1cs;
using namespace cwc_g16;
using namespace cwc_kzg;

constexpr int KZG_PHASES = 4;   // quotient, lincomb, prepare, pairing
constexpr int FOLD_PHASES = 6;  // fold, evals, quotient, lincomb, prepare, pairing: a folded call, in the order it enqueues them

struct gwb_kzg {
    gwb_kzg_info_t info{};
    int device = -1;
    std::vector<uint8_t> lagrange;  // section 12 as stored, the levels 0 .. top_level (empty for a file that is not prepared)
    uint32_t top_level = 0;         // the largest m with 2^m <= max_len
    std::string unprepared;         // need_prepared's message for this file
    std::vector<uint8_t> srs, tau_g2;  // T_0 .. T_{max_len-1} and tauG2, canonical, until they are on the device
    DeviceBuf d_srs, d_tau_g2;      // the same there, from the first call that runs on the device
    std::map<uint32_t, DeviceBuf> d_lag;  // level m of section 12, canonical
    Workspace ws;
    // the last open or verify call: one set of events per sub-batch, and the phases that enqueued nothing
    std::mutex mutex;
    std::vector<PhaseEvents<KZG_PHASES + 1>> events;
    uint32_t idle = 0;
    // the same of the last open_fold or verify_fold call
    std::vector<PhaseEvents<FOLD_PHASES + 1>> fold_events;
    uint32_t fold_idle = 0;
};

namespace {

std::string status_text(gw_status_t& st, const char* fallback) {
    std::string m = st.error_msg ? st.error_msg : fallback;
    free(st.error_msg);
    st.error_msg = nullptr;
    return m;
}

// n stored points at `stored` (section `section`, the first of them its point `base`) -> canonical bytes; the host checks first
bool canonical_points(uint32_t section, uint64_t base, const uint8_t* stored, uint64_t n, std::vector<uint8_t>& out, std::string& err) {
    out.resize(n * G1_BYTES);
    for (uint64_t i = 0; i < n; ++i) {
        const PointFault f = point_fault<G1>(stored + i * G1_BYTES, false);
        if (f != PointFault::NONE) {
            err = cwc_ptau::point_message(section, base + i, f, false);
            return false;
        }
        cwc_contrib::canonical_g1(stored + i * G1_BYTES, out.data() + i * G1_BYTES);
    }
    return true;
}

// The powers check over what covers max_len points of section 2: gwb_ptau_check_powers for the smallest domain n with 2n >= max_len,
// and where the file has no such domain (max_len > 2^power) the whole file's sums and equations.
bool check_powers(const uint8_t* data, size_t len, const cwc_ptau::View& v, uint64_t max_len, std::string& err) {
    uint32_t p = 0;
    while ((2ull << p) < max_len) ++p;
    gw_status_t st{};
    if (p + 1 <= v.power) {
        if (gwb_ptau_check_powers(data, len, p, nullptr, &st) == 0) {
            free(st.error_msg);
            return true;
        }
        err = status_text(st, "ptau: the powers check failed");
        return false;
    }
    const uint64_t np = 1ull << v.power;
    cwc_ptau::Plan pl;
    pl.p = v.power;
    pl.t1 = v.sec[2].p;
    pl.t2 = v.sec[3].p;
    pl.at = v.sec[4].p;
    pl.bt = v.sec[5].p;
    pl.beta2 = v.sec[6].p;
    if (!cwc_ptau::check_all_points(v, err)) return false;
    std::string msg;
    if (cwc_ptau::check_g2_points(6, 0, v.sec[6].p, 1, msg) != 0 || cwc_ptau::check_g2_points(3, 0, v.sec[3].p, np, msg) != 0) {
        err = msg;
        return false;
    }
    uint8_t seed[32];
    if (!cwc_contrib::seed_or_draw(nullptr, seed)) {
        err = "ptau: getrandom failed";
        return false;
    }
    cwc_contrib::PowersSums sums;
    std::vector<cwc_contrib::PairCheck> checks;
    std::string host_verdict, verdict;
    if (!cwc_contrib::powers_rules(pl, np, 2 * np - 2, true, seed, sums, checks, host_verdict, err) || !cwc_contrib::run_pair_checks(checks, verdict, err)) return false;
    if (verdict.empty()) verdict = host_verdict;
    err = verdict;
    return verdict.empty();
}

int make_handle(const uint8_t* data, size_t len, uint64_t max_len, uint32_t flags, gwb_kzg_t** out, gw_status_t* status) {
    if (flags & ~(uint32_t)GWB_KZG_CHECK_POWERS) return fail(status, "kzg: unknown flags " + std::to_string(flags));
    if (max_len == 0) return fail(status, "kzg: max_len is 0");
    std::string err;
    cwc_ptau::View v;
    if (!cwc_ptau::parse(data, len, v, err)) return fail(status, err);
    const uint64_t points = (2ull << v.power) - 1;
    if (max_len > points)
        return fail(status, "kzg: max_len " + std::to_string(max_len) + " is above the 2^(power+1) - 1 = " + std::to_string(points) + " points of tauG1 in a file of power " +
                                std::to_string(v.power));
    std::unique_ptr<gwb_kzg> h(new gwb_kzg);
    std::vector<uint8_t>&srs = h->srs, &tau2 = h->tau_g2;
    tau2.resize(G2_BYTES);
    if (!canonical_points(2, 0, v.sec[2].p, max_len, srs, err)) return fail(status, err);
    const uint8_t* t2_1 = v.sec[3].p + G2_BYTES;
    const PointFault f2 = point_fault<G2>(t2_1, false);
    if (f2 != PointFault::NONE) return fail(status, cwc_ptau::point_message(3, 1, f2, true));
    cwc_contrib::canonical_g2(t2_1, tau2.data());
    if (std::all_of(tau2.begin(), tau2.end(), [](uint8_t b) { return b == 0; })) return fail(status, "kzg: tauG2[1] is the point at infinity");
    h->info.max_len = max_len;
    h->info.power = v.power;
    h->info.prepared = v.prepared ? 1 : 0;
    while ((2ull << h->top_level) <= max_len) ++h->top_level;
    if (v.prepared)
        h->lagrange.assign(v.sec[12].p, v.sec[12].p + ((2ull << h->top_level) - 1) * G1_BYTES);
    else
        cwc_ptau::need_prepared(v, h->unprepared);
    // -- the device only when the powers check is asked for; the points go there at the first call that needs them (on_device)
    if ((flags & GWB_KZG_CHECK_POWERS) && !check_powers(data, len, v, max_len, err)) return fail(status, err);
    *out = h.release();
    set_ok(status);
    return 0;
}

// The points are on the current device: they go there at the first call, and later calls have to be on that device.
bool on_device(gwb_kzg* h, std::string& err) {
    std::lock_guard<std::mutex> lock(h->mutex);
    if (!h->d_srs) {
        hipError_t e = hipGetDevice(&h->device);
        if (e == hipSuccess) e = h->d_srs.upload(h->srs.data(), h->srs.size());
        if (e == hipSuccess) e = h->d_tau_g2.upload(h->tau_g2.data(), h->tau_g2.size());
        if (e != hipSuccess) {
            h->d_srs.reset();
            err = hip_err("uploading the KZG reference string", e);
            return false;
        }
        std::vector<uint8_t>().swap(h->srs);
        return true;
    }
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == h->device) return true;
    err = "kzg: the handle's points are on device " + std::to_string(h->device) + ", the current device is " + std::to_string(cur);
    return false;
}

bool fits(const gwb_kzg* h, size_t N, std::string& err) {
    if (N <= h->info.max_len) return true;
    err = "kzg: a polynomial of " + std::to_string(N) + " coefficients is above the handle's max_len " + std::to_string(h->info.max_len);
    return false;
}

// out[k] = sum_i scalars[k][i] bases[i] for K rows of N scalars (any value below 2^256: a multiple of r times a point of G1 is O)
bool enqueue_commits(const uint8_t* d_bases, const uint8_t* d_scalars, size_t K, size_t N, uint8_t* d_out, hipStream_t s, std::string& err) {
    for (size_t k = 0; k < K; ++k) {
        gw_status_t st{};
        if (gwb_bn254_g1_lincomb_device(d_bases, d_scalars + k * N * 32, N, GWB_FORM_CANONICAL, d_out + k * G1_BYTES, s, &st) != 0) {
            err = status_text(st, "kzg: the linear combination failed");
            return false;
        }
    }
    return true;
}

// the Lagrange points of level m on the device, uploaded at the first call for that m
bool lagrange_level(gwb_kzg* h, uint32_t m, const uint8_t** d_lag, std::string& err) {
    if (!h->info.prepared) {
        err = h->unprepared;
        return false;
    }
    if (m > h->top_level) {
        err = "kzg: 2^" + std::to_string(m) + " evaluations are above the handle's max_len " + std::to_string(h->info.max_len);
        return false;
    }
    if (!on_device(h, err)) return false;
    std::lock_guard<std::mutex> lock(h->mutex);
    DeviceBuf& buf = h->d_lag[m];
    if (!buf) {
        const uint64_t first = (1ull << m) - 1, n = 1ull << m;
        std::vector<uint8_t> pts;
        if (!canonical_points(12, first, h->lagrange.data() + first * G1_BYTES, n, pts, err)) return false;
        const hipError_t e = buf.upload(pts.data(), pts.size());
        if (e != hipSuccess) {
            err = hip_err("uploading a Lagrange level of the KZG reference string", e);
            return false;
        }
    }
    *d_lag = buf.as<uint8_t>();
    return true;
}

// fresh events for a call of `subs` sub-batches (a failure leaves timing off for the call)
template <class Events>
void start_phases(gwb_kzg* h, Events& events, uint32_t& idle_out, size_t subs, uint32_t idle) {
    std::lock_guard<std::mutex> lock(h->mutex);
    events.clear();
    events.resize(subs);
    idle_out = idle;
    for (auto& ev : events)
        if (ev.on() != hipSuccess) {
            events.clear();
            break;
        }
}
void start_phases(gwb_kzg* h, size_t subs, uint32_t idle) { start_phases(h, h->events, h->idle, subs, idle); }
void start_fold_phases(gwb_kzg* h, size_t subs, uint32_t idle) { start_phases(h, h->fold_events, h->fold_idle, subs, idle); }
void mark(const gwb_kzg* h, size_t sub, int i, hipStream_t s) {
    if (sub < h->events.size()) h->events[sub].record(i, s);
}
void mark_fold(const gwb_kzg* h, size_t sub, int i, hipStream_t s) {
    if (sub < h->fold_events.size()) h->fold_events[sub].record(i, s);
}

// ms[PHASES] of the call whose events these are, summed over its sub-batches; the phases of `idle` are 0
template <int PHASES>
int phase_ms(gwb_kzg* h, const std::vector<PhaseEvents<PHASES + 1>>& events, uint32_t idle, float* ms) {
    std::lock_guard<std::mutex> lock(h->mutex);
    if (events.empty()) return 1;
    float sum[PHASES] = {};
    for (const auto& ev : events) {
        float t[PHASES];
        if (ev.elapsed(t) != hipSuccess) return 1;
        for (int i = 0; i < PHASES; ++i) sum[i] += (idle >> i) & 1u ? 0.0f : t[i];
    }
    memcpy(ms, sum, sizeof sum);
    return 0;
}

bool open_device(gwb_kzg* h, const uint8_t* d_polys, const uint8_t* d_zs, size_t K, size_t N, uint8_t* d_ys, uint8_t* d_proofs, hipStream_t s,
                 std::string& err) {
    if ((d_proofs && !fits(h, N, err)) || !on_device(h, err)) return false;
    if (N > 0x7fffffffull) {
        err = "kzg: a polynomial of more than 2^31 - 1 coefficients";
        return false;
    }
    if (K == 0) return true;
    if (N == 0) {
        hipError_t e = hipMemsetAsync(d_ys, 0, K * 32, s);
        if (e == hipSuccess && d_proofs) e = hipMemsetAsync(d_proofs, 0, K * G1_BYTES, s);
        if (e != hipSuccess) err = hip_err("zeroing the openings of empty polynomials", e);
        return e == hipSuccess;
    }
    const bool quotient = d_proofs && N > 1;
    const size_t q_bytes = quotient ? (N - 1) * 32 : 0;
    const uint64_t per_pair = q_bytes + eval_quotient_ws(1, N, TILE_PRODUCTION);
    const size_t sub = (size_t)std::min<uint64_t>(K, std::max<uint64_t>(1, groth16_workspace_cap() / per_pair));
    Carve cw;
    const size_t o_q = cw.take(sub * q_bytes), o_lv = cw.take(eval_quotient_ws(sub, N, TILE_PRODUCTION));
    if (!h->ws.ensure(cw.o, "allocating the KZG workspace", err)) return false;
    uint8_t* W = h->ws.as<uint8_t>();
    if (d_proofs) start_phases(h, (K + sub - 1) / sub, 0xcu);
    for (size_t at = 0, i = 0; at < K; at += sub, ++i) {
        const size_t k = std::min(sub, K - at);
        mark(h, i, 0, s);
        if (!enqueue_eval_quotient(d_polys + at * N * 32, d_zs + at * 32, 1, k, (uint32_t)N, TILE_PRODUCTION, d_ys + at * 32, quotient ? W + o_q : nullptr, W + o_lv, s, err))
            return false;
        mark(h, i, 1, s);
        if (d_proofs && !enqueue_commits(h->d_srs.as<uint8_t>(), W + o_q, k, N - 1, d_proofs + at * G1_BYTES, s, err)) return false;
        for (int e = 2; e <= KZG_PHASES; ++e) mark(h, i, e, s);
    }
    return true;
}

constexpr size_t VERIFY_ROW_BYTES = 2 * (G1_BYTES + G2_BYTES + GWB_GT_BYTES);
// the pairing's own workspace per opening, which it allocates itself in stream order: verify.hip's pairing_ws for two pairs (320 bytes
// of points, an Fq12 and eight Fq12 spill slots each)
constexpr size_t PAIRING_ROW_ESTIMATE = 2 * (320 + 9 * 384);

bool verify_device(gwb_kzg* h, const uint8_t* d_c, const uint8_t* d_z, const uint8_t* d_y, const uint8_t* d_w, size_t K, uint32_t* d_status, hipStream_t s,
                   std::string& err) {
    if (!on_device(h, err)) return false;
    if (K == 0) return true;
    const size_t sub = (size_t)std::min<uint64_t>(std::min<uint64_t>(K, (1u << 30) - 1), std::max<uint64_t>(1, groth16_workspace_cap() / (VERIFY_ROW_BYTES + PAIRING_ROW_ESTIMATE)));
    Carve cw;
    const size_t o_g1 = cw.take(sub * 2 * G1_BYTES), o_g2 = cw.take(sub * 2 * G2_BYTES), o_gt = cw.take(sub * 2 * GWB_GT_BYTES);
    if (!h->ws.ensure(cw.o, "allocating the KZG workspace", err)) return false;
    uint8_t* W = h->ws.as<uint8_t>();
    start_phases(h, (K + sub - 1) / sub, 0x3u);
    for (size_t at = 0, i = 0; at < K; at += sub, ++i) {
        const uint32_t k = (uint32_t)std::min(sub, K - at);
        for (int e = 0; e <= 2; ++e) mark(h, i, e, s);
        if (!enqueue_prepare(d_c + at * G1_BYTES, d_z + at * 32, d_y + at * 32, d_w + at * G1_BYTES, k, h->d_tau_g2.as<uint8_t>(), W + o_g1, W + o_g2, d_status + at, s, err))
            return false;
        mark(h, i, 3, s);
        gw_status_t st{};
        if (gwb_bn254_pairing_batch_device(W + o_g1, W + o_g2, 2 * (size_t)k, W + o_gt, s, &st) != 0) {
            err = status_text(st, "kzg: the pairing failed");
            return false;
        }
        if (!enqueue_compare(W + o_gt, k, d_status + at, s, err)) return false;
        mark(h, i, 4, s);
    }
    return true;
}

// What every folded call refuses about G groups of K, before the device is touched
bool fold_shape(size_t G, size_t K, std::string& err) {
    if (K == 0) {
        err = "kzg: a group of 0 polynomials";
        return false;
    }
    size_t pairs = 0;
    if (__builtin_mul_overflow(G, K, &pairs) || pairs > MAX_FOLD_PAIRS) {
        err = "kzg: " + std::to_string(G) + " groups of " + std::to_string(K) + " are more than 2^31 - 1 (polynomial, point) pairs";
        return false;
    }
    return true;
}

bool open_fold_device(gwb_kzg* h, const uint8_t* d_polys, const uint8_t* d_zs, const uint8_t* d_gammas, size_t G, size_t K, size_t N, uint8_t* d_ys,
                      uint8_t* d_proofs, hipStream_t s, std::string& err) {
    if (!fold_shape(G, K, err) || !fits(h, N, err)) return false;
    if (N > 0x7fffffffull) {
        err = "kzg: a polynomial of more than 2^31 - 1 coefficients";
        return false;
    }
    if (G == 0) return true;
    if (!on_device(h, err)) return false;
    if (N == 0) {
        hipError_t e = hipMemsetAsync(d_ys, 0, G * K * 32, s);
        if (e == hipSuccess) e = hipMemsetAsync(d_proofs, 0, G * G1_BYTES, s);
        if (e != hipSuccess) err = hip_err("zeroing the openings of empty polynomials", e);
        return e == hipSuccess;
    }
    // per group: the folded polynomial, its quotient and its value, and the levels of its K evaluations (the quotient's pass has fewer pairs)
    const bool quotient = N > 1;
    const size_t f_bytes = quotient ? N * 32 : 0, q_bytes = quotient ? (N - 1) * 32 : 0;
    const uint64_t per_group = f_bytes + q_bytes + 32 + K * eval_quotient_ws(1, N, TILE_PRODUCTION);
    const size_t sub = (size_t)std::min<uint64_t>(G, std::max<uint64_t>(1, groth16_workspace_cap() / per_group));
    Carve cw;
    const size_t o_f = cw.take(sub * f_bytes), o_q = cw.take(sub * q_bytes), o_yf = cw.take(sub * 32), o_lv = cw.take(eval_quotient_ws(sub * K, N, TILE_PRODUCTION));
    if (!h->ws.ensure(cw.o, "allocating the KZG workspace", err)) return false;
    uint8_t* W = h->ws.as<uint8_t>();
    start_fold_phases(h, (G + sub - 1) / sub, 0x30u);
    for (size_t at = 0, i = 0; at < G; at += sub, ++i) {
        const size_t g = std::min(sub, G - at);
        const uint8_t* polys = d_polys + at * K * N * 32;
        mark_fold(h, i, 0, s);
        if (quotient && !enqueue_fold(polys, d_gammas + at * 32, g, (uint32_t)K, (uint32_t)N, W + o_f, s, err)) return false;
        mark_fold(h, i, 1, s);
        if (!enqueue_eval_quotient(polys, d_zs + at * 32, (uint32_t)K, g * K, (uint32_t)N, TILE_PRODUCTION, d_ys + at * K * 32, nullptr, W + o_lv, s, err)) return false;
        mark_fold(h, i, 2, s);
        if (quotient && !enqueue_eval_quotient(W + o_f, d_zs + at * 32, 1, g, (uint32_t)N, TILE_PRODUCTION, W + o_yf, W + o_q, W + o_lv, s, err)) return false;
        mark_fold(h, i, 3, s);
        if (quotient) {
            if (!enqueue_commits(h->d_srs.as<uint8_t>(), W + o_q, g, N - 1, d_proofs + at * G1_BYTES, s, err)) return false;
        } else {
            const hipError_t e = hipMemsetAsync(d_proofs + at * G1_BYTES, 0, g * G1_BYTES, s);
            if (e != hipSuccess) {
                err = hip_err("zeroing the witnesses of constant polynomials", e);
                return false;
            }
        }
        for (int e = 4; e <= FOLD_PHASES; ++e) mark_fold(h, i, e, s);
    }
    return true;
}

bool verify_fold_device(gwb_kzg* h, const uint8_t* d_c, const uint8_t* d_z, const uint8_t* d_gammas, const uint8_t* d_y, const uint8_t* d_w, size_t G, size_t K,
                        uint32_t* d_status, hipStream_t s, std::string& err) {
    if (!fold_shape(G, K, err)) return false;
    if (G == 0) return true;
    if (!on_device(h, err)) return false;
    const uint64_t row = VERIFY_ROW_BYTES + PAIRING_ROW_ESTIMATE + fold_points_ws(1, (uint32_t)K, true);
    const size_t sub = (size_t)std::min<uint64_t>(std::min<uint64_t>(G, (1u << 30) - 1), std::max<uint64_t>(1, groth16_workspace_cap() / row));
    Carve cw;
    const size_t o_g1 = cw.take(sub * 2 * G1_BYTES), o_g2 = cw.take(sub * 2 * G2_BYTES), o_gt = cw.take(sub * 2 * GWB_GT_BYTES),
                 o_part = cw.take(fold_points_ws(sub, (uint32_t)K, true));
    if (!h->ws.ensure(cw.o, "allocating the KZG workspace", err)) return false;
    uint8_t* W = h->ws.as<uint8_t>();
    start_fold_phases(h, (G + sub - 1) / sub, 0xfu);
    for (size_t at = 0, i = 0; at < G; at += sub, ++i) {
        const uint32_t g = (uint32_t)std::min(sub, G - at);
        const uint8_t* w = d_w + at * G1_BYTES;
        for (int e = 0; e <= 4; ++e) mark_fold(h, i, e, s);
        if (!enqueue_fold_points(d_c + at * K * G1_BYTES, d_gammas + at * 32, d_z + at * 32, d_y + at * K * 32, w, g, (uint32_t)K, W + o_part, s, err) ||
            !enqueue_fold_emit(W + o_part, w, g, (uint32_t)K, h->d_tau_g2.as<uint8_t>(), W + o_g1, W + o_g2, d_status + at, s, err))
            return false;
        mark_fold(h, i, 5, s);
        gw_status_t st{};
        if (gwb_bn254_pairing_batch_device(W + o_g1, W + o_g2, 2 * (size_t)g, W + o_gt, s, &st) != 0) {
            err = status_text(st, "kzg: the pairing failed");
            return false;
        }
        if (!enqueue_compare(W + o_gt, g, d_status + at, s, err)) return false;
        mark_fold(h, i, 6, s);
    }
    return true;
}

int done(bool ok, const std::string& err, gw_status_t* status) {
    if (!ok) return fail(status, err);
    set_ok(status);
    return 0;
}

}  // namespace

extern "C" {

int gwb_kzg_new(const void* ptau, size_t len, uint64_t max_len, uint32_t flags, gwb_kzg_t** out, gw_status_t* status) {
    if (!out || (!ptau && len)) return fail(status, "gwb_kzg_new: NULL argument");
    *out = nullptr;
    try {
        return make_handle((const uint8_t*)ptau, len, max_len, flags, out, status);
    } catch (const std::bad_alloc&) {
        return fail(status, "kzg: out of host memory");
    }
}

int gwb_kzg_info(const gwb_kzg_t* h, gwb_kzg_info_t* info) {
    if (!h || !info) return 1;
    *info = h->info;
    return 0;
}

void gwb_kzg_free(gwb_kzg_t* h) { delete h; }

int gwb_kzg_commit_batch_device(gwb_kzg_t* h, const void* d_polys, size_t K, size_t N, void* d_points, void* hip_stream, gw_status_t* status) {
    if (!h || (K && (!d_points || (N && !d_polys)))) return fail(status, "gwb_kzg_commit_batch_device: NULL argument");
    std::string err;
    return done(fits(h, N, err) && on_device(h, err) && enqueue_commits(h->d_srs.as<uint8_t>(), (const uint8_t*)d_polys, K, N, (uint8_t*)d_points, (hipStream_t)hip_stream, err),
                err, status);
}

int gwb_kzg_commit_batch(gwb_kzg_t* h, const void* polys, size_t K, size_t N, void* points, gw_status_t* status) {
    if (!h || (K && (!points || (N && !polys)))) return fail(status, "gwb_kzg_commit_batch: NULL argument");
    std::string err;
    if (!fits(h, N, err)) return fail(status, err);
    auto run = [&](unsigned char* const* d, hipStream_t s, std::string& e) {
        return on_device(h, e) && enqueue_commits(h->d_srs.as<uint8_t>(), d[0], K, N, d[1], s, e);
    };
    return done(K == 0 || run_staged({K * N * 32, K * G1_BYTES}, {{polys, K * N * 32, 0, 0}}, {{points, K * G1_BYTES, 1, 0}}, "staging the polynomials",
                                     "running the KZG commitments", run, err),
                err, status);
}

int gwb_kzg_commit_evals_batch_device(gwb_kzg_t* h, const void* d_evals, size_t K, uint32_t m, void* d_points, void* hip_stream, gw_status_t* status) {
    if (!h || (K && (!d_points || !d_evals))) return fail(status, "gwb_kzg_commit_evals_batch_device: NULL argument");
    std::string err;
    const uint8_t* d_lag = nullptr;
    return done(lagrange_level(h, m, &d_lag, err) && enqueue_commits(d_lag, (const uint8_t*)d_evals, K, (size_t)1 << m, (uint8_t*)d_points, (hipStream_t)hip_stream, err),
                err, status);
}

int gwb_kzg_commit_evals_batch(gwb_kzg_t* h, const void* evals, size_t K, uint32_t m, void* points, gw_status_t* status) {
    if (!h || (K && (!points || !evals))) return fail(status, "gwb_kzg_commit_evals_batch: NULL argument");
    std::string err;
    if (!h->info.prepared) return fail(status, h->unprepared);
    if (m > h->top_level) return fail(status, "kzg: 2^" + std::to_string(m) + " evaluations are above the handle's max_len " + std::to_string(h->info.max_len));
    const size_t N = (size_t)1 << m;
    auto run = [&](unsigned char* const* d, hipStream_t s, std::string& e) {
        const uint8_t* d_lag = nullptr;
        return lagrange_level(h, m, &d_lag, e) && enqueue_commits(d_lag, d[0], K, N, d[1], s, e);
    };
    return done(K == 0 || run_staged({K * N * 32, K * G1_BYTES}, {{evals, K * N * 32, 0, 0}}, {{points, K * G1_BYTES, 1, 0}}, "staging the evaluations",
                                     "running the KZG commitments", run, err),
                err, status);
}

int gwb_kzg_eval_batch_device(gwb_kzg_t* h, const void* d_polys, const void* d_zs, size_t K, size_t N, void* d_ys, void* hip_stream, gw_status_t* status) {
    if (!h || (K && (!d_zs || !d_ys || (N && !d_polys)))) return fail(status, "gwb_kzg_eval_batch_device: NULL argument");
    std::string err;
    return done(open_device(h, (const uint8_t*)d_polys, (const uint8_t*)d_zs, K, N, (uint8_t*)d_ys, nullptr, (hipStream_t)hip_stream, err), err, status);
}

int gwb_kzg_eval_batch(gwb_kzg_t* h, const void* polys, const void* zs, size_t K, size_t N, void* ys, gw_status_t* status) {
    if (!h || (K && (!zs || !ys || (N && !polys)))) return fail(status, "gwb_kzg_eval_batch: NULL argument");
    std::string err;
    auto run = [&](unsigned char* const* d, hipStream_t s, std::string& e) { return open_device(h, d[0], d[1], K, N, d[2], nullptr, s, e); };
    return done(K == 0 || run_staged({K * N * 32, K * 32, K * 32}, {{polys, K * N * 32, 0, 0}, {zs, K * 32, 1, 0}}, {{ys, K * 32, 2, 0}}, "staging the polynomials",
                                     "running the KZG evaluations", run, err),
                err, status);
}

int gwb_kzg_open_batch_device(gwb_kzg_t* h, const void* d_polys, const void* d_zs, size_t K, size_t N, void* d_ys, void* d_proofs, void* hip_stream,
                              gw_status_t* status) {
    if (!h || (K && (!d_zs || !d_ys || !d_proofs || (N && !d_polys)))) return fail(status, "gwb_kzg_open_batch_device: NULL argument");
    std::string err;
    return done(open_device(h, (const uint8_t*)d_polys, (const uint8_t*)d_zs, K, N, (uint8_t*)d_ys, (uint8_t*)d_proofs, (hipStream_t)hip_stream, err), err, status);
}

int gwb_kzg_open_batch(gwb_kzg_t* h, const void* polys, const void* zs, size_t K, size_t N, void* ys, void* proofs, gw_status_t* status) {
    if (!h || (K && (!zs || !ys || !proofs || (N && !polys)))) return fail(status, "gwb_kzg_open_batch: NULL argument");
    std::string err;
    if (!fits(h, N, err)) return fail(status, err);
    auto run = [&](unsigned char* const* d, hipStream_t s, std::string& e) { return open_device(h, d[0], d[1], K, N, d[2], d[3], s, e); };
    return done(K == 0 || run_staged({K * N * 32, K * 32, K * 32, K * G1_BYTES}, {{polys, K * N * 32, 0, 0}, {zs, K * 32, 1, 0}},
                                     {{ys, K * 32, 2, 0}, {proofs, K * G1_BYTES, 3, 0}}, "staging the polynomials", "running the KZG openings", run, err),
                err, status);
}

int gwb_kzg_verify_batch_device(gwb_kzg_t* h, const void* d_commitments, const void* d_zs, const void* d_ys, const void* d_proofs, size_t K, void* d_status,
                                void* hip_stream, gw_status_t* status) {
    if (!h || (K && (!d_commitments || !d_zs || !d_ys || !d_proofs || !d_status))) return fail(status, "gwb_kzg_verify_batch_device: NULL argument");
    std::string err;
    return done(verify_device(h, (const uint8_t*)d_commitments, (const uint8_t*)d_zs, (const uint8_t*)d_ys, (const uint8_t*)d_proofs, K, (uint32_t*)d_status,
                              (hipStream_t)hip_stream, err),
                err, status);
}

int gwb_kzg_verify_batch(gwb_kzg_t* h, const void* commitments, const void* zs, const void* ys, const void* proofs, size_t K, void* status_out,
                         gw_status_t* status) {
    if (!h || (K && (!commitments || !zs || !ys || !proofs || !status_out))) return fail(status, "gwb_kzg_verify_batch: NULL argument");
    std::string err;
    Carve c;  // one allocation: the commitments, the points, the values, the proofs, the statuses
    const size_t o_c = c.take(K * G1_BYTES), o_z = c.take(K * 32), o_y = c.take(K * 32), o_w = c.take(K * G1_BYTES), o_st = c.take(K * 4);
    auto run = [&](unsigned char* const* d, hipStream_t s, std::string& e) {
        return verify_device(h, d[0] + o_c, d[0] + o_z, d[0] + o_y, d[0] + o_w, K, (uint32_t*)(d[0] + o_st), s, e);
    };
    return done(K == 0 || run_staged({c.o}, {{commitments, K * G1_BYTES, 0, o_c}, {zs, K * 32, 0, o_z}, {ys, K * 32, 0, o_y}, {proofs, K * G1_BYTES, 0, o_w}},
                                     {{status_out, K * 4, 0, o_st}}, "staging the openings", "running the KZG opening check", run, err),
                err, status);
}

int gwb_kzg_open_fold_batch_device(gwb_kzg_t* h, const void* d_polys, const void* d_zs, const void* d_gammas, size_t G, size_t K, size_t N, void* d_ys,
                                   void* d_proofs, void* hip_stream, gw_status_t* status) {
    if (!h || (G && K && (!d_zs || !d_gammas || !d_ys || !d_proofs || (N && !d_polys)))) return fail(status, "gwb_kzg_open_fold_batch_device: NULL argument");
    std::string err;
    return done(open_fold_device(h, (const uint8_t*)d_polys, (const uint8_t*)d_zs, (const uint8_t*)d_gammas, G, K, N, (uint8_t*)d_ys, (uint8_t*)d_proofs,
                                 (hipStream_t)hip_stream, err),
                err, status);
}

int gwb_kzg_open_fold_batch(gwb_kzg_t* h, const void* polys, const void* zs, const void* gammas, size_t G, size_t K, size_t N, void* ys, void* proofs,
                            gw_status_t* status) {
    if (!h || (G && K && (!zs || !gammas || !ys || !proofs || (N && !polys)))) return fail(status, "gwb_kzg_open_fold_batch: NULL argument");
    std::string err;
    if (!fold_shape(G, K, err) || !fits(h, N, err)) return fail(status, err);
    Carve c;  // one allocation for the points and the challenges
    const size_t o_z = c.take(G * 32), o_g = c.take(G * 32);
    auto run = [&](unsigned char* const* d, hipStream_t s, std::string& e) { return open_fold_device(h, d[0], d[1] + o_z, d[1] + o_g, G, K, N, d[2], d[3], s, e); };
    return done(G == 0 || run_staged({G * K * N * 32, c.o, G * K * 32, G * G1_BYTES}, {{polys, G * K * N * 32, 0, 0}, {zs, G * 32, 1, o_z}, {gammas, G * 32, 1, o_g}},
                                     {{ys, G * K * 32, 2, 0}, {proofs, G * G1_BYTES, 3, 0}}, "staging the polynomials", "running the folded KZG openings", run, err),
                err, status);
}

int gwb_kzg_verify_fold_batch_device(gwb_kzg_t* h, const void* d_commitments, const void* d_zs, const void* d_gammas, const void* d_ys, const void* d_proofs,
                                     size_t G, size_t K, void* d_status, void* hip_stream, gw_status_t* status) {
    if (!h || (G && K && (!d_commitments || !d_zs || !d_gammas || !d_ys || !d_proofs || !d_status)))
        return fail(status, "gwb_kzg_verify_fold_batch_device: NULL argument");
    std::string err;
    return done(verify_fold_device(h, (const uint8_t*)d_commitments, (const uint8_t*)d_zs, (const uint8_t*)d_gammas, (const uint8_t*)d_ys, (const uint8_t*)d_proofs, G,
                                   K, (uint32_t*)d_status, (hipStream_t)hip_stream, err),
                err, status);
}

int gwb_kzg_verify_fold_batch(gwb_kzg_t* h, const void* commitments, const void* zs, const void* gammas, const void* ys, const void* proofs, size_t G, size_t K,
                              void* status_out, gw_status_t* status) {
    if (!h || (G && K && (!commitments || !zs || !gammas || !ys || !proofs || !status_out))) return fail(status, "gwb_kzg_verify_fold_batch: NULL argument");
    std::string err;
    if (!fold_shape(G, K, err)) return fail(status, err);
    Carve c;  // one allocation: the commitments, the points, the challenges, the values, the proofs, the statuses
    const size_t o_c = c.take(G * K * G1_BYTES), o_z = c.take(G * 32), o_g = c.take(G * 32), o_y = c.take(G * K * 32), o_w = c.take(G * G1_BYTES),
                 o_st = c.take(G * 4);
    auto run = [&](unsigned char* const* d, hipStream_t s, std::string& e) {
        return verify_fold_device(h, d[0] + o_c, d[0] + o_z, d[0] + o_g, d[0] + o_y, d[0] + o_w, G, K, (uint32_t*)(d[0] + o_st), s, e);
    };
    return done(G == 0 || run_staged({c.o},
                                     {{commitments, G * K * G1_BYTES, 0, o_c}, {zs, G * 32, 0, o_z}, {gammas, G * 32, 0, o_g}, {ys, G * K * 32, 0, o_y},
                                      {proofs, G * G1_BYTES, 0, o_w}},
                                     {{status_out, G * 4, 0, o_st}}, "staging the folded openings", "running the folded KZG opening check", run, err),
                err, status);
}

int gwb_kzg_fold_device(const void* d_polys, const void* d_gammas, size_t G, size_t K, size_t N, void* d_out, void* hip_stream, gw_status_t* status) {
    std::string err;
    if (!fold_shape(G, K, err)) return fail(status, err);
    if (N > 0x7fffffffull) return fail(status, "gwb_kzg_fold_device: N above 2^31 - 1");
    if (G == 0 || N == 0) return done(true, "", status);
    if (!d_polys || !d_gammas || !d_out) return fail(status, "gwb_kzg_fold_device: NULL argument");
    return done(enqueue_fold((const uint8_t*)d_polys, (const uint8_t*)d_gammas, G, (uint32_t)K, (uint32_t)N, (uint8_t*)d_out, (hipStream_t)hip_stream, err), err, status);
}

int gwb_kzg_fold_points_device(const void* d_points, const void* d_gammas, size_t G, size_t K, void* d_out, void* hip_stream, gw_status_t* status) {
    std::string err;
    if (!fold_shape(G, K, err)) return fail(status, err);
    if (G == 0) return done(true, "", status);
    if (!d_points || !d_gammas || !d_out) return fail(status, "gwb_kzg_fold_points_device: NULL argument");
    hipStream_t s = (hipStream_t)hip_stream;
    Carve c;  // the partial sums, and the first group with a refused point
    const size_t o_part = c.take(fold_points_ws(G, (uint32_t)K, false)), o_fault = c.take(4);
    void* ws = nullptr;
    hipError_t e = hipMallocAsync(&ws, c.o, s);
    if (e != hipSuccess) return fail(status, hip_err("allocating the point fold's workspace", e));
    uint8_t* W = (uint8_t*)ws;
    uint32_t fault = 0xffffffffu;
    e = hipMemsetAsync(W + o_fault, 0xff, 4, s);
    bool ok = e == hipSuccess && enqueue_fold_points((const uint8_t*)d_points, (const uint8_t*)d_gammas, nullptr, nullptr, nullptr, G, (uint32_t)K, W + o_part, s, err) &&
              enqueue_fold_sum(W + o_part, (uint32_t)G, (uint32_t)K, (uint8_t*)d_out, (uint32_t*)(W + o_fault), s, err);
    if (ok) e = hipMemcpyAsync(&fault, W + o_fault, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (the one wait: the refusal below needs the kernels' finding)
    const hipError_t ef = hipFreeAsync(ws, s);
    if (e == hipSuccess) e = ef;
    if (err.empty() && e != hipSuccess) err = hip_err("running the point fold", e);
    if (err.empty() && fault != 0xffffffffu)
        err = "kzg: a point of group " + std::to_string(fault) + " has a coordinate at or above q, or is neither on the curve nor the point at infinity";
    return done(err.empty(), err, status);
}

int gwb_kzg_phase_ms(gwb_kzg_t* h, float* ms) {
    if (!h || !ms) return 1;
    return phase_ms<KZG_PHASES>(h, h->events, h->idle, ms);
}

int gwb_kzg_fold_phase_ms(gwb_kzg_t* h, float* ms) {
    if (!h || !ms) return 1;
    return phase_ms<FOLD_PHASES>(h, h->fold_events, h->fold_idle, ms);
}

int gwb_kzg_eval_quotient_device(const void* d_polys, const void* d_zs, size_t K, size_t N, uint32_t tile, void* d_ys, void* d_qs, void* hip_stream,
                                 gw_status_t* status) {
    if (tile == 0) tile = TILE_PRODUCTION;
    if (!tile_ok(tile)) return fail(status, "gwb_kzg_eval_quotient_device: tile " + std::to_string(tile) + " is not instantiated (gwb_kzg_tiles)");
    if (K && (!d_zs || !d_ys || (N && !d_polys) || (N > 1 && !d_qs))) return fail(status, "gwb_kzg_eval_quotient_device: NULL argument");
    if (N > 0x7fffffffull) return fail(status, "gwb_kzg_eval_quotient_device: N above 2^31 - 1");
    hipStream_t s = (hipStream_t)hip_stream;
    if (K == 0) return done(true, "", status);
    if (N == 0) {
        const hipError_t e = hipMemsetAsync(d_ys, 0, K * 32, s);
        return done(e == hipSuccess, hip_err("zeroing the values of empty polynomials", e), status);
    }
    void* ws = nullptr;
    hipError_t e = hipMallocAsync(&ws, eval_quotient_ws(K, N, tile), s);
    if (e != hipSuccess) return fail(status, hip_err("allocating the evaluate-and-quotient workspace", e));
    std::string err;
    const bool ok = enqueue_eval_quotient((const uint8_t*)d_polys, (const uint8_t*)d_zs, 1, K, (uint32_t)N, tile, (uint8_t*)d_ys, N > 1 ? (uint8_t*)d_qs : nullptr, (uint8_t*)ws, s, err);
    e = hipFreeAsync(ws, s);
    if (ok && e != hipSuccess) err = hip_err("releasing the evaluate-and-quotient workspace", e);
    return done(ok && e == hipSuccess, err, status);
}

int gwb_kzg_tiles(uint32_t* tiles, size_t* n) {
    if (!n) return 1;
    const uint32_t all[2] = {TILE_SMALL, TILE_PRODUCTION};
    for (size_t i = 0; i < 2 && i < *n && tiles; ++i) tiles[i] = all[i];
    *n = 2;
    return 0;
}

}  // extern "C"
