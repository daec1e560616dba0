// Groth16 witness map on gfx950 (include/graph_witness_r1cs.h has the definition): per witness row, the QAP rows a, b and
// c = a b on the domain of n = 2^p points, three inverse NTTs, the coset shift g^i, three forward NTTs and
// h = A B - C at the coset points.  Every internal value is in Montgomery form.
//
// Buffers per sub-batch of rows: A and B in the handle's workspace, C in the caller's h ([row][n] each).  The evaluation
// kernel writes a, b and c at each constraint's file index (the check's lane mapping and factor stream, lincomb.hpp); a
// second kernel writes the input rows and the zero padding.
//
// The map runs over a RowSystem (r1cs_internal.hpp), whichever source it came from: an `.r1cs`, or a zkey's section 4 when a
// prover has none (include/graph_witness_groth16.h; the arrays zkey_coefs.cc builds).  The sources differ in the row-pointer
// stride, a template parameter of the evaluation kernel, and in the rows above the evaluated ones: after an `.r1cs` they are
// the input rows taken from the witness and zeros (qap_pad_kernel), while section 4 has the public rows among its entries and
// the rest is cleared (qap_zero_kernel).  The tables, workspace and events of the NTT chain are the row system's QapState.
//
// NTT layout: n = L_0 L_1 ... L_{P-1} (each L <= 2^9 for the outer passes, the innermost <= 2^11).  A pass works on blocks
// of M = L S consecutive elements (S = L_{t+1} ... L_{P-1}): position k S + j (k < L, j < S) of a block is element k of
// column j.  An inverse pass takes the L-point DFT (root w_L^-1) of every column and multiplies element k of column j by
// w_M^-(k j) (four-step / Bailey form, with the transposes left out).  Run outermost first, the inverse passes leave
// coefficient k_0 + L_0 (k_1 + L_1 (...)) at position k_0 (n / L_0) + k_1 (n / L_0 L_1) + ... (digits reversed): the
// coset table holds g^i / n for the coefficient i at each position.  A forward pass is the transpose of an inverse one
// (twiddle w_M^(k j) first, then the DFT with root w_L), run innermost first, so it consumes that order and produces
// natural order.  The innermost inverse pass, the coset scaling and the innermost forward pass are one kernel; the last
// forward pass also forms A B - C and the output form, in place in h.
//
// A pass's block of threads takes tiles of L x Cc elements (Cc = min(S, 4) adjacent columns: 128 contiguous bytes per
// column element) into 64 KiB of LDS, in bit-reversed order inside each column, and runs the radix-2 DIT stages there;
// small transforms put several tiles in one block.  The twiddles are read from a resident table of w_n^e.
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "lincomb.hpp"
#include "groth16_internal.hpp"
#include "hip_util.hpp"
#include "r1cs_internal.hpp"

using namespace cwc_r1cs;
using cwc::Fr;

namespace {

constexpr uint32_t MAX_POWER = MAX_DOMAIN_POWER;
constexpr uint32_t LOG_TILE = 11;      // elements per block (LDS: 2^11 x 32 B = 64 KiB)
constexpr uint32_t LOG_OUTER_MAX = 9;  // outer passes: L <= 2^9, 4 columns
constexpr uint32_t LOG_COLS = 2;
constexpr uint32_t THREADS = 256;
constexpr uint32_t PER_THREAD = (1u << LOG_TILE) / THREADS;
constexpr int EVAL_WAVES = 4;

// The pass structure of a domain: log2 L_t, outermost first; the last entry is the innermost (S = 1) pass.
struct Plan {
    uint32_t p = 0, n_pass = 0;
    uint32_t logl[4] = {0, 0, 0, 0};
};

Plan make_plan(uint32_t p) {
    Plan pl;
    pl.p = p;
    const uint32_t inner = std::min(p, LOG_TILE), rest = p - inner;
    const uint32_t m = (rest + LOG_OUTER_MAX - 1) / LOG_OUTER_MAX;  // at most 2 for p <= 27
    for (uint32_t t = 0; t < m; ++t) pl.logl[t] = rest / m + (t < rest % m ? 1 : 0);
    pl.logl[m] = inner;
    pl.n_pass = m + 1;
    return pl;
}

// tw[e] = w_n^e; coset[pos] = g^i / n for the coefficient i the inverse passes leave at pos (digits of pos reversed)
__global__ __launch_bounds__(THREADS) void qap_tables_kernel(Fr* __restrict__ tw, Fr* __restrict__ coset, uint32_t log_n, Pows w_pows,
                                                             Pows g_pows, Fr n_inv, Plan plan) {
    const uint32_t n = 1u << log_n;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        Fr t = cwc::fr_one();
        for (uint32_t b = 0; b < log_n; ++b)
            if ((e >> b) & 1u) t = cwc::fr_mul(t, w_pows.v[b]);
        tw[e] = t;
        uint32_t idx = 0, shift = 0, rem = e, lsize = log_n;
        for (uint32_t k = 0; k < plan.n_pass; ++k) {
            lsize -= plan.logl[k];
            idx |= (rem >> lsize) << shift;
            shift += plan.logl[k];
            rem &= (1u << lsize) - 1u;
        }
        Fr c = n_inv;
        for (uint32_t b = 0; b < log_n; ++b)
            if ((idx >> b) & 1u) c = cwc::fr_mul(c, g_pows.v[b]);
        coset[e] = c;
    }
}

__device__ __forceinline__ Fr to_internal(Fr w, uint32_t montgomery) {
    w = reduce_any(w);
    return montgomery ? w : cwc::fr_to_mont(w);
}

// a and b of rows [0, n_rows) (constraint index perm[c]) into A and B, c = a b into C; the check kernel's lane mapping.
// STRIDE row pointers per row: 3 for an `.r1cs` (the C side is not read), 2 for section 4.
template <int T, int STRIDE>
__global__ __launch_bounds__(64 * EVAL_WAVES) void qap_eval_kernel(
    const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ fac, const uint32_t* __restrict__ cidx, const Fr* __restrict__ coef,
    const uint32_t* __restrict__ perm, uint32_t n_rows, const uint8_t* __restrict__ witness, uint32_t n_witness, uint32_t batch,
    uint32_t montgomery, Fr* __restrict__ A, Fr* __restrict__ B, Fr* __restrict__ C, uint32_t log_n) {
    constexpr uint32_t G = 64 / T;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t set = blockIdx.x * T + lane % T;
    const bool set_ok = set < batch;
    if (!set_ok) set = batch - 1;
    const uint8_t* row = witness + (size_t)set * n_witness * 32;
    const size_t out_row = (size_t)set << log_n;
    const uint32_t n_groups = (n_rows + G - 1) / G;
    for (uint32_t g = blockIdx.y * EVAL_WAVES + wave; g < n_groups; g += gridDim.y * EVAL_WAVES) {
        uint32_t c = g * G + lane / T;
        const bool c_ok = c < n_rows;
        if (!c_ok) c = n_rows - 1;  // (n_rows >= 1: the host launches nothing for a system without rows)
        const uint32_t ka = rowptr[STRIDE * c], kb = rowptr[STRIDE * c + 1], kc = rowptr[STRIDE * c + 2];
        Fr a = lin_comb(fac, cidx, coef, ka, kb, row);
        Fr b = lin_comb(fac, cidx, coef, kb, kc, row);
        if (!montgomery) {  // canonical row: the sums are canonical
            a = cwc::fr_to_mont(a);
            b = cwc::fr_to_mont(b);
        }
        const Fr ab = cwc::fr_mul(a, b);
        if (set_ok && c_ok) {
            const size_t o = out_row + perm[c];
            A[o] = a;
            B[o] = b;
            C[o] = ab;
        }
    }
}

// section 4: rows n_used .. n-1 of every set: a = b = c = 0 (n_used < n: the caller skips the launch otherwise)
__global__ __launch_bounds__(THREADS) void qap_zero_kernel(uint32_t batch, uint32_t n_used, Fr* __restrict__ A, Fr* __restrict__ B,
                                                           Fr* __restrict__ C, uint32_t log_n) {
    const uint64_t per = (1ull << log_n) - n_used, total = per * batch;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t set = k / per, s = k % per;
        const size_t o = (set << log_n) + n_used + s;
        A[o] = cwc::fr_zero();
        B[o] = cwc::fr_zero();
        C[o] = cwc::fr_zero();
    }
}

// `.r1cs`: rows nC .. n-1 of every set: a = w[i - nC] for i - nC <= nPub, else 0; b = c = 0
__global__ __launch_bounds__(THREADS) void qap_pad_kernel(const uint8_t* __restrict__ witness, uint32_t n_witness, uint32_t batch,
                                                          uint32_t montgomery, uint32_t n_constraints, uint32_t n_pub, Fr* __restrict__ A,
                                                          Fr* __restrict__ B, Fr* __restrict__ C, uint32_t log_n) {
    const uint64_t per = (1ull << log_n) - n_constraints, total = per * batch;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t set = k / per, s = k % per;
        const size_t o = (set << log_n) + n_constraints + s;
        A[o] = s <= n_pub ? to_internal(load_elem(witness + set * n_witness * 32, (uint32_t)s), montgomery) : cwc::fr_zero();
        B[o] = cwc::fr_zero();
        C[o] = cwc::fr_zero();
    }
}

struct PassArgs {
    Fr* arr[3];  // A, B, C (C is the output h)
    const Fr* tw;
    const Fr* coset;
    uint32_t log_n, log_l, log_s, log_cc, log_units;  // 2^log_units tiles of L x Cc per block
    uint32_t tiles_per_row;
    uint64_t n_tiles;    // rows x tiles_per_row
    uint32_t combine;    // last forward pass: h = A B - C into arr[2]
    uint32_t mont_out;
};

enum { PASS_INV = 0, PASS_MID = 1, PASS_FWD = 2 };

// radix-2 DIT stages over every column of the block's LDS image (columns of L elements, bit-reversed in, natural out)
template <bool INV>
__device__ __forceinline__ void lds_dft(Fr* lds, uint32_t n_bfly, uint32_t log_l, const Fr* __restrict__ tw, uint32_t log_n) {
    const uint32_t mask = (1u << log_n) - 1u, half = log_l - 1;
    for (uint32_t lh = 0; lh < log_l; ++lh) {
        const uint32_t h = 1u << lh;
        for (uint32_t b = threadIdx.x; b < n_bfly; b += THREADS) {
            const uint32_t col = b >> half, r = b & ((1u << half) - 1u), k = r & (h - 1u);
            const uint32_t i0 = (col << log_l) + ((r >> lh) << (lh + 1)) + k, i1 = i0 + h;
            const Fr u = lds[i0];
            Fr v = lds[i1];
            if (lh) {
                uint32_t e = k << (log_n - lh - 1);  // w_(2h)^k = w_n^(k n / 2h)
                if (INV) e = (0u - e) & mask;
                v = cwc::fr_mul(v, tw[e]);
            }
            lds[i0] = cwc::fr_add(u, v);
            lds[i1] = cwc::fr_sub(u, v);
        }
        __syncthreads();
    }
}

template <int KIND>
__global__ __launch_bounds__(THREADS) void qap_pass_kernel(PassArgs a) {
    __shared__ Fr lds[1u << LOG_TILE];
    const uint32_t log_e = a.log_l + a.log_cc, n_elem = 1u << (log_e + a.log_units);
    const uint32_t mask = (1u << a.log_n) - 1u, tw_shift = a.log_n - a.log_l - a.log_s;
    const uint64_t tile0 = (uint64_t)blockIdx.x << a.log_units;
    // this thread's elements: global offset, LDS slot (natural and bit-reversed inside its column), column, k
    size_t off[PER_THREAD];
    uint32_t nat[PER_THREAD], rev[PER_THREAD], kj[PER_THREAD];
    bool ok[PER_THREAD];
#pragma unroll
    for (uint32_t i = 0; i < PER_THREAD; ++i) {
        const uint32_t e = threadIdx.x + i * THREADS;
        const uint64_t tile = tile0 + (e >> log_e);
        ok[i] = e < n_elem && tile < a.n_tiles;
        const uint32_t local = e & ((1u << log_e) - 1u);
        const uint32_t c = local & ((1u << a.log_cc) - 1u), k = local >> a.log_cc;
        const uint64_t row = tile / a.tiles_per_row;
        const uint32_t t = (uint32_t)(tile % a.tiles_per_row);
        const uint32_t log_groups = a.log_s - a.log_cc;
        const uint32_t blk = t >> log_groups, j = ((t & ((1u << log_groups) - 1u)) << a.log_cc) + c;
        off[i] = (size_t)(row << a.log_n) + ((size_t)blk << (a.log_l + a.log_s)) + ((size_t)k << a.log_s) + j;
        const uint32_t base = ((e >> log_e) << log_e) + (c << a.log_l);  // this column's run of L slots in the LDS image
        nat[i] = base + k;
        rev[i] = base + (a.log_l ? __brev(k) >> (32 - a.log_l) : 0u);
        kj[i] = k * j;  // < M
    }
    const uint32_t n_bfly = n_elem >> 1;
    Fr keep[PER_THREAD];
    for (int q = 0; q < 3; ++q) {
        Fr* arr = a.arr[q];
#pragma unroll
        for (uint32_t i = 0; i < PER_THREAD; ++i) {
            if (!ok[i]) continue;
            Fr x = arr[off[i]];
            if (KIND == PASS_FWD && kj[i]) x = cwc::fr_mul(x, a.tw[(kj[i] << tw_shift) & mask]);
            lds[rev[i]] = x;
        }
        __syncthreads();
        lds_dft<KIND != PASS_FWD>(lds, n_bfly, a.log_l, a.tw, a.log_n);
        if (KIND == PASS_MID) {  // coefficients: scale by g^i / n, back to bit-reversed order, forward DFT
            Fr x[PER_THREAD];
#pragma unroll
            for (uint32_t i = 0; i < PER_THREAD; ++i)
                if (ok[i]) x[i] = cwc::fr_mul(lds[nat[i]], a.coset[off[i] & mask]);
            __syncthreads();
#pragma unroll
            for (uint32_t i = 0; i < PER_THREAD; ++i)
                if (ok[i]) lds[rev[i]] = x[i];
            __syncthreads();
            lds_dft<false>(lds, n_bfly, a.log_l, a.tw, a.log_n);
        }
#pragma unroll
        for (uint32_t i = 0; i < PER_THREAD; ++i) {
            if (!ok[i]) continue;
            Fr x = lds[nat[i]];
            if (KIND == PASS_INV && kj[i]) x = cwc::fr_mul(x, a.tw[(0u - (kj[i] << tw_shift)) & mask]);
            if (!a.combine) {
                arr[off[i]] = x;
            } else if (q == 0) {
                keep[i] = x;
            } else if (q == 1) {
                keep[i] = cwc::fr_mul(keep[i], x);
            } else {
                Fr h = cwc::fr_sub(keep[i], x);
                if (!a.mont_out) h = cwc::fr_mul(h, Fr{{1, 0, 0, 0, 0, 0, 0, 0}});
                arr[off[i]] = h;
            }
        }
        __syncthreads();  // the next array reuses the LDS image
    }
}

// measurement aid: chained Montgomery products, 4 independent chains per lane (gwb_r1cs_modmul_rate)
__global__ __launch_bounds__(THREADS) void modmul_probe_kernel(Fr* __restrict__ out, uint32_t iters) {
    Fr x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = Fr{{blockIdx.x * THREADS + threadIdx.x + 1u + (uint32_t)i, 7u, 0, 0, 0, 0, 0, 1u}};
    const Fr m = Fr{{0x12345u, 0x6789u, 3u, 0, 0, 0, 0, 5u}};
    for (uint32_t k = 0; k < iters; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = cwc::fr_mul(x[i], m);
    out[blockIdx.x * THREADS + threadIdx.x] = cwc::fr_add(cwc::fr_add(x[0], x[1]), cwc::fr_add(x[2], x[3]));
}

typedef void (*EvalFn)(const uint32_t*, const uint32_t*, const uint32_t*, const Fr*, const uint32_t*, uint32_t, const uint8_t*, uint32_t,
                       uint32_t, uint32_t, Fr*, Fr*, Fr*, uint32_t);

template <int STRIDE>
EvalFn eval_of(uint32_t t) {
    switch (t) {
        case 1: return qap_eval_kernel<1, STRIDE>;
        case 2: return qap_eval_kernel<2, STRIDE>;
        case 4: return qap_eval_kernel<4, STRIDE>;
        case 8: return qap_eval_kernel<8, STRIDE>;
        case 16: return qap_eval_kernel<16, STRIDE>;
        case 32: return qap_eval_kernel<32, STRIDE>;
        default: return qap_eval_kernel<64, STRIDE>;
    }
}

EvalFn eval_for(uint32_t t, uint32_t stride) { return stride == 3 ? eval_of<3>(t) : eval_of<2>(t); }

struct Domain {
    uint64_t n_rows = 0;
    uint32_t p = 0;
};

bool domain_of(const gwb_r1cs* r, Domain& d, std::string& err) {
    d.n_rows = (uint64_t)r->info.n_constraints + r->info.n_pub_out + r->info.n_pub_in + 1;
    d.p = 1;
    while ((1ull << d.p) < d.n_rows) ++d.p;
    if (d.p > MAX_POWER) {
        err = "r1cs: the QAP domain needs 2^" + std::to_string(d.p) + " points for " + std::to_string(d.n_rows) +
              " rows; at most 2^27 are supported (the coset needs a 2n-th root of unity and r has 2-adicity 28)";
        return false;
    }
    return true;
}

uint64_t ws_per_row(uint32_t p) { return 2ull * 32 << p; }  // A and B

// workspace cap in bytes: CWC_R1CS_QAP_WORKSPACE_MB, read once per process
uint64_t ws_cap() {
    static const uint64_t cap = [] {
        const char* s = getenv("CWC_R1CS_QAP_WORKSPACE_MB");
        const unsigned long long mb = s && *s ? strtoull(s, nullptr, 10) : 0ull;
        return (mb ? (uint64_t)mb : 4096ull) << 20;
    }();
    return cap;
}

Fr fr_pow(Fr base_m, const Fr& e) {  // Montgomery in and out
    Fr acc = cwc::fr_one();
    for (int b = 255; b >= 0; --b) {
        acc = cwc::fr_mul(acc, acc);
        if ((e.v[b >> 5] >> (b & 31)) & 1u) acc = cwc::fr_mul(acc, base_m);
    }
    return acc;
}

}  // namespace

namespace cwc_r1cs {
// w_28 = 5^((r-1) / 2^28); w_n = w_28^(2^(28-p)); g = w_28^(2^(27-p)); Montgomery form
void qap_roots(uint32_t p, Fr& wn, Fr& g) {
    Fr rm1 = cwc::fr_p();
    rm1.v[0] -= 1;  // r is odd
    g = fr_pow(cwc::fr_to_mont(Fr{{5, 0, 0, 0, 0, 0, 0, 0}}), cwc::u256_shr(rm1, 28));
    for (uint32_t i = 0; i < MAX_POWER - p; ++i) g = cwc::fr_mul(g, g);
    wn = cwc::fr_mul(g, g);
}
}  // namespace cwc_r1cs

namespace {

// twiddle and coset tables of the handle's domain, on its device (synchronous, first call only)
bool ensure_tables(QapState& st, uint32_t p, std::string& err) {
    if (st.tw) return true;
    const uint64_t n = 1ull << p;
    Fr rm1 = cwc::fr_p();
    rm1.v[0] -= 1;  // r is odd
    Fr wn, g;
    qap_roots(p, wn, g);
    // 1/n = r - (r-1)/n, since n divides r - 1
    Fr q = cwc::u256_shr(rm1, p), n_inv;
    cwc::u256_sub(n_inv, cwc::fr_p(), q);
    n_inv = cwc::fr_to_mont(n_inv);
    DeviceBuf tw, cs;
    Stream s;
    hipError_t e = tw.alloc(n * 32);
    if (e == hipSuccess) e = cs.alloc(n * 32);
    if (e == hipSuccess) e = s.create();
    if (e == hipSuccess) {
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + THREADS - 1) / THREADS, 4096);
        hipLaunchKernelGGL(qap_tables_kernel, dim3(blocks), dim3(THREADS), 0, s, tw.as<Fr>(), cs.as<Fr>(), p, powers_of(wn), powers_of(g), n_inv, make_plan(p));
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) {
        err = hip_err("building the QAP twiddle tables", e);
        return false;
    }
    st.tw = std::move(tw);
    st.coset = std::move(cs);
    return true;
}

bool launch_pass(int kind, PassArgs a, uint64_t rows, hipStream_t stream, std::string& err) {
    const uint32_t log_e = a.log_l + a.log_cc;
    a.tiles_per_row = 1u << (a.log_n - log_e);
    a.n_tiles = rows * a.tiles_per_row;
    a.log_units = LOG_TILE - log_e;
    const uint64_t blocks = (a.n_tiles + (1ull << a.log_units) - 1) >> a.log_units;
    if (blocks > 0x7fffffffull) {
        err = "r1cs: QAP sub-batch too large for one launch";
        return false;
    }
    auto fn = kind == PASS_INV ? qap_pass_kernel<PASS_INV> : kind == PASS_MID ? qap_pass_kernel<PASS_MID> : qap_pass_kernel<PASS_FWD>;
    hipLaunchKernelGGL(fn, dim3((uint32_t)blocks), dim3(THREADS), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        err = hip_err("launching a QAP NTT pass", e);
        return false;
    }
    return true;
}

// The NTT chain over `rows` rows of evaluations (A, B in the workspace, C in d_h): three inverse transforms, the coset
// shift, three forward transforms and h = A B - C into d_h.  Records the state's phase events 1 to 4.
bool transform(QapState& q, uint32_t p, Fr* A, Fr* B, Fr* d_h, uint64_t rows, uint32_t form_out, hipStream_t stream, std::string& err) {
    q.events.record(1, stream);
    const Plan pl = make_plan(p);
    PassArgs a{};
    a.arr[0] = A;
    a.arr[1] = B;
    a.arr[2] = d_h;
    a.tw = q.tw.as<const Fr>();
    a.coset = q.coset.as<const Fr>();
    a.log_n = p;
    a.mont_out = form_out == GWB_FORM_MONTGOMERY ? 1u : 0u;
    uint32_t log_s[4], below = p;
    for (uint32_t t = 0; t < pl.n_pass; ++t) log_s[t] = (below -= pl.logl[t]);
    const uint32_t outer = pl.n_pass - 1;
    for (uint32_t t = 0; t < outer; ++t) {
        a.log_l = pl.logl[t];
        a.log_s = log_s[t];
        a.log_cc = std::min(LOG_COLS, log_s[t]);
        a.combine = 0;
        if (!launch_pass(PASS_INV, a, rows, stream, err)) return false;
    }
    q.events.record(2, stream);
    a.log_l = pl.logl[outer];
    a.log_s = 0;
    a.log_cc = 0;
    a.combine = outer == 0;
    if (!launch_pass(PASS_MID, a, rows, stream, err)) return false;
    q.events.record(3, stream);
    for (uint32_t t = outer; t-- > 0;) {
        a.log_l = pl.logl[t];
        a.log_s = log_s[t];
        a.log_cc = std::min(LOG_COLS, log_s[t]);
        a.combine = t == 0;
        if (!launch_pass(PASS_FWD, a, rows, stream, err)) return false;
    }
    q.events.record(4, stream);
    return true;
}

// One witness map: the rows, the domain of 2^p points, and what else the sources differ in
struct Map {
    RowSystem* sys = nullptr;
    uint32_t p = 0;
    uint32_t n_pub = 0;  // `.r1cs`: rows n_rows .. n_rows + n_pub are the first witness elements (qap_pad_kernel)
    int home = -1;       // the device the arrays have to share (ensure_device)
};

bool map_of(gwb_r1cs* r, Map& m, std::string& err) {
    Domain d;
    if (!domain_of(r, d, err)) return false;
    m = Map{&r->sys, d.p, r->info.n_pub_out + r->info.n_pub_in, -1};
    return true;
}

// (domainSize is a power of two in 2 .. 2^27 once the map is built; the arrays go where the zkey's points are, if uploaded)
bool map_of(gwb_zkey* z, Map& m, std::string& err) {
    if (!zkey_coefs_build(z, err)) return false;
    uint32_t p = 0;
    while ((1u << p) < z->info.domain_size) ++p;
    m = Map{&z->sys, p, 0, z->device};
    return true;
}

// h of `rows` rows: d_w rows -> A, B (workspace), C = d_h -> h in d_h
bool enqueue_sub(const Map& m, const uint8_t* d_w, uint64_t rows, uint32_t form_in, Fr* d_h, uint32_t form_out, hipStream_t stream,
                 std::string& err) {
    RowSystem& s = *m.sys;
    const uint32_t p = m.p, nr = s.n_rows, nw = s.n_wires;
    const uint64_t n = 1ull << p;
    Fr* A = s.qap.ws.as<Fr>();
    Fr* B = A + rows * n;
    const uint32_t mont = form_in == GWB_FORM_MONTGOMERY ? 1u : 0u;
    s.qap.events.record(0, stream);
    const int cus = cu_count(s.device);
    if (nr) {  // (an `.r1cs` may have no constraints; section 4 has at least one row)
        EvalGrid g;
        if (!eval_grid(s, rows, cus, EVAL_WAVES, g, err)) return false;
        hipLaunchKernelGGL(eval_for(g.t, s.stride), dim3(g.tiles, g.gy), dim3(64 * EVAL_WAVES), 0, stream, s.d_rowptr.as<const uint32_t>(),
                           s.d_fac.as<const uint32_t>(), s.d_cidx.as<const uint32_t>(), s.d_coef.as<const Fr>(), s.d_perm.as<const uint32_t>(), nr, d_w, nw,
                           (uint32_t)rows, mont, A, B, d_h, p);
    }
    // the rows above: the one difference between the sources
    const uint64_t pad = (n - nr) * rows;
    const uint32_t pad_blocks = (uint32_t)std::min<uint64_t>((pad + THREADS - 1) / THREADS, (uint64_t)cus * 16);
    if (s.stride == 3)  // (never empty: the row of wire 0 follows the constraints)
        hipLaunchKernelGGL(qap_pad_kernel, dim3(pad_blocks), dim3(THREADS), 0, stream, d_w, nw, (uint32_t)rows, mont, nr, m.n_pub, A, B, d_h, p);
    else if (pad)  // n_used == n (nC + nPublic + 1 a power of two): no row is left to clear, and a grid of 0 blocks is no launch
        hipLaunchKernelGGL(qap_zero_kernel, dim3(pad_blocks), dim3(THREADS), 0, stream, (uint32_t)rows, nr, A, B, d_h, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        err = hip_err("launching the QAP evaluation", e);
        return false;
    }
    return transform(s.qap, p, A, B, d_h, rows, form_out, stream, err);
}

bool form_ok(uint32_t f) { return f == GWB_FORM_CANONICAL || f == GWB_FORM_MONTGOMERY; }

// device rows -> d_h, in sub-batches under the workspace cap
bool enqueue_qap(const Map& m, const void* d_witness, size_t batch, uint32_t form_in, void* d_h, uint32_t form_out, hipStream_t stream,
                 std::string& err) {
    RowSystem& s = *m.sys;
    if (!ensure_device(s, m.home, err) || !ensure_tables(s.qap, m.p, err)) return false;
    const uint64_t per = ws_per_row(m.p);
    const uint64_t sub = std::min<uint64_t>(batch, std::max<uint64_t>(1, ws_cap() / per));
    if (!s.qap.ws.ensure(sub * per, "allocating the QAP workspace", err)) return false;
    const uint64_t n = 1ull << m.p;
    for (uint64_t s0 = 0; s0 < batch; s0 += sub) {
        const uint64_t rows = std::min<uint64_t>(sub, batch - s0);
        if (!enqueue_sub(m, (const uint8_t*)d_witness + s0 * s.n_wires * 32, rows, form_in, (Fr*)d_h + s0 * n, form_out, stream, err)) return false;
    }
    return true;
}

// host rows -> device -> h back; synchronous
int qap_host(const Map& m, const void* witness, size_t n_witness, size_t batch, void* h, uint32_t form_out, gw_status_t* status) {
    std::string err;
    if (!check_args(*m.sys, n_witness, batch, err)) return fail(status, err);
    if (batch == 0) {
        set_ok(status);
        return 0;
    }
    if (!ensure_device(*m.sys, m.home, err)) return fail(status, err);
    const size_t wbytes = batch * n_witness * 32, hbytes = (batch * 32) << m.p;
    auto run = [&](unsigned char* const* d, hipStream_t s, std::string& err) {
        return enqueue_qap(m, d[0], batch, GWB_FORM_CANONICAL, d[1], form_out, s, err);
    };
    if (!run_staged({wbytes, hbytes}, {{witness, wbytes, 0, 0}}, {{h, hbytes, 1, 0}}, "staging the witness rows", "running the QAP witness map", run, err))
        return fail(status, err);
    set_ok(status);
    return 0;
}

// The bodies of gwb_r1cs_qap_batch_* and gwb_zkey_qap_batch_*; `fn` is the entry point's name
template <class H>
int batch_device(const char* fn, H* h, const void* d_witness, size_t n_witness, size_t batch, uint32_t form_in, void* d_h, uint32_t form_out,
                 void* hip_stream, gw_status_t* status) {
    if (!h || (batch && (!d_witness || !d_h))) return fail(status, std::string(fn) + ": NULL argument");
    if (!form_ok(form_in)) return fail(status, std::string(fn) + ": unknown form " + std::to_string(form_in));
    if (!form_ok(form_out)) return fail(status, std::string(fn) + ": unknown form " + std::to_string(form_out));
    std::string err;
    Map m;
    if (!map_of(h, m, err) || !check_args(*m.sys, n_witness, batch, err)) return fail(status, err);
    if (batch == 0) {
        set_ok(status);
        return 0;
    }
    if (!enqueue_qap(m, d_witness, batch, form_in, d_h, form_out, (hipStream_t)hip_stream, err)) return fail(status, err);
    set_ok(status);
    return 0;
}

template <class H>
int batch_host(const char* fn, H* handle, const void* witness, size_t n_witness, size_t batch, void* h, uint32_t form_out, gw_status_t* status) {
    if (!handle || (batch && (!witness || !h))) return fail(status, std::string(fn) + ": NULL argument");
    if (!form_ok(form_out)) return fail(status, std::string(fn) + ": unknown form " + std::to_string(form_out));
    std::string err;
    Map m;
    if (!map_of(handle, m, err)) return fail(status, err);
    return qap_host(m, witness, n_witness, batch, h, form_out, status);
}

}  // namespace

namespace cwc_r1cs {

bool qap_enqueue(gwb_r1cs* r, const void* d_witness, size_t batch, uint32_t form_in, void* d_h, uint32_t form_out, void* stream,
                 std::string& err) {
    Map m;
    return map_of(r, m, err) && enqueue_qap(m, d_witness, batch, form_in, d_h, form_out, (hipStream_t)stream, err);
}

bool qap_enqueue(gwb_zkey* z, const void* d_witness, size_t batch, uint32_t form_in, void* d_h, uint32_t form_out, void* stream,
                 std::string& err) {
    Map m;
    return map_of(z, m, err) && enqueue_qap(m, d_witness, batch, form_in, d_h, form_out, (hipStream_t)stream, err);
}

}  // namespace cwc_r1cs

extern "C" {

int gwb_r1cs_qap_info(const gwb_r1cs_t* r, gwb_r1cs_qap_info_t* info, gw_status_t* status) {
    if (!r || !info) return fail(status, "gwb_r1cs_qap_info: NULL argument");
    Domain d;
    std::string err;
    if (!domain_of(r, d, err)) return fail(status, err);
    info->n_rows = d.n_rows;
    info->domain_power = d.p;
    info->domain_size = 1ull << d.p;
    info->workspace_bytes_per_row = ws_per_row(d.p);
    set_ok(status);
    return 0;
}

int gwb_r1cs_qap_batch_device(gwb_r1cs_t* r, const void* d_witness, size_t n_witness, size_t batch, uint32_t form_in, void* d_h,
                              uint32_t form_out, void* hip_stream, gw_status_t* status) {
    return batch_device("gwb_r1cs_qap_batch_device", r, d_witness, n_witness, batch, form_in, d_h, form_out, hip_stream, status);
}

int gwb_r1cs_qap_batch_host(gwb_r1cs_t* r, const void* witness, size_t n_witness, size_t batch, void* h, uint32_t form_out, gw_status_t* status) {
    return batch_host("gwb_r1cs_qap_batch_host", r, witness, n_witness, batch, h, form_out, status);
}

int gwb_r1cs_qap_wtns(gwb_r1cs_t* r, const void* wtns, size_t len, void* h_out, uint32_t form_out, gw_status_t* status) {
    if (!r || !wtns || !h_out) return fail(status, "gwb_r1cs_qap_wtns: NULL argument");
    if (!form_ok(form_out)) return fail(status, "gwb_r1cs_qap_wtns: unknown form " + std::to_string(form_out));
    const uint8_t* values = nullptr;
    uint64_t n_wit = 0;
    std::string err;
    Map m;
    if (!parse_wtns(wtns, len, &values, &n_wit, err) || !map_of(r, m, err)) return fail(status, err);
    return qap_host(m, values, n_wit, 1, h_out, form_out, status);
}

int gwb_zkey_qap_batch_device(gwb_zkey_t* z, const void* d_witness, size_t n_witness, size_t batch, uint32_t form_in, void* d_h,
                              uint32_t form_out, void* hip_stream, gw_status_t* status) {
    return batch_device("gwb_zkey_qap_batch_device", z, d_witness, n_witness, batch, form_in, d_h, form_out, hip_stream, status);
}

int gwb_zkey_qap_batch_host(gwb_zkey_t* z, const void* witness, size_t n_witness, size_t batch, void* h, uint32_t form_out, gw_status_t* status) {
    return batch_host("gwb_zkey_qap_batch_host", z, witness, n_witness, batch, h, form_out, status);
}

int gwb_r1cs_qap_time_phases(gwb_r1cs_t* r, int on) {
    if (!r) return 1;
    if (!on) r->sys.qap.events.off();
    return on && r->sys.qap.events.on() != hipSuccess ? 1 : 0;
}

int gwb_r1cs_modmul_rate(double* products_per_s) {
    if (!products_per_s) return 1;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        return 1;
    const uint32_t blocks = (uint32_t)cus * 8, iters = 4096;  // 8 waves per SIMD
    DeviceBuf out;
    PhaseEvents<2> ev;
    hipError_t e = out.alloc((size_t)blocks * THREADS * 32);
    if (e == hipSuccess) e = ev.on();
    float ms[1] = {0};
    if (e == hipSuccess) {
        hipLaunchKernelGGL(modmul_probe_kernel, dim3(blocks), dim3(THREADS), 0, nullptr, out.as<Fr>(), 16u);  // warm-up
        ev.record(0, nullptr);
        hipLaunchKernelGGL(modmul_probe_kernel, dim3(blocks), dim3(THREADS), 0, nullptr, out.as<Fr>(), iters);
        ev.record(1, nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = ev.elapsed(ms);
    }
    if (e != hipSuccess || ms[0] <= 0) return 1;
    *products_per_s = (double)blocks * THREADS * 4 * iters / (ms[0] * 1e-3);
    return 0;
}

int gwb_r1cs_qap_phase_ms(gwb_r1cs_t* r, float* ms) {
    float t[4];
    if (!r || !ms || r->sys.qap.events.elapsed(t) != hipSuccess) return 1;
    memcpy(ms, t, sizeof t);
    return 0;
}

}  // extern "C"
