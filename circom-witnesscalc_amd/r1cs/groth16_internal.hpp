// Host representation of a loaded `.zkey` (zkey.cc), shared with the prover (msm.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/graph_witness_groth16.h"
#include "r1cs_internal.hpp"

constexpr size_t G1_BYTES = 64, G2_BYTES = 128;

struct gwb_zkey {
    gwb_zkey_info_t info{};
    // affine points as stored (x, y; x.c0, x.c1, y.c0, y.c1), Montgomery form mod q, all-zero = infinity
    uint8_t alpha1[G1_BYTES], beta1[G1_BYTES], delta1[G1_BYTES], beta2[G2_BYTES], gamma2[G2_BYTES], delta2[G2_BYTES];
    std::vector<uint8_t> ic, a, b1, b2, c, h;  // sections 3, 5, 6, 7, 8, 9
    // device copies (first prove call): A, B1, B2 with two more points each, the bases of the scalars r and s
    // (A: delta1, O; B1: O, delta1; B2: O, delta2), then C and H as stored
    int device = -1;
    void *d_a = nullptr, *d_b1 = nullptr, *d_b2 = nullptr, *d_c = nullptr, *d_h = nullptr;
    void* d_ws = nullptr;
    size_t ws_bytes = 0;
    void* h_rs = nullptr;  // pinned staging of r, s (h_rs_bytes), and the event after its last copy
    size_t h_rs_bytes = 0;
    void* rs_done = nullptr;
    void* events[8] = {};  // phase timing (gwb_groth16_time_phases): recorded around each phase of the last sub-batch
    // Section 4 as stored (n_coefs x 44 B: u32 matrix, constraint, signal, then the value c R^2 mod r), bounds-checked at load.
    std::vector<uint8_t> sec4;
    // The witness map of section 4 (zkey_coefs.cc, built at the first call that needs it), in the layout of gwb_r1cs without
    // the C side: row k's A factors are fac[rowptr[2k] .. rowptr[2k+1]), B up to rowptr[2k+2]; perm[k] = its constraint
    // index; rows bucketed by length.  n_used = 1 + the largest constraint index of any entry.
    bool coefs_built = false;
    uint32_t n_used = 0;
    std::vector<uint32_t> rowptr, fac, cidx, perm;
    std::vector<cwc::Fr> coef;  // distinct general coefficients, Montgomery form c R
    uint32_t tile_width = 0;    // 0 = from the batch size
    // device copies of the arrays above (first zkey QAP call) and the domain's state (qap.hip)
    int qap_device = -1;
    void *d_rowptr = nullptr, *d_fac = nullptr, *d_cidx = nullptr, *d_coef = nullptr, *d_perm = nullptr;
    cwc_r1cs::QapState qap;
};

namespace cwc_r1cs {
// qap.hip: the witness map of device rows into d_h, as gwb_r1cs_qap_batch_device enqueues it (arguments checked by the caller)
bool qap_enqueue(gwb_r1cs* r, const void* d_witness, size_t batch, uint32_t form_in, void* d_h, uint32_t form_out, void* stream,
                 std::string& err);
// zkey_coefs.cc: builds the witness map of section 4 (first call; later calls return at once).  Refusals start "zkey:".
bool zkey_coefs_build(gwb_zkey* z, std::string& err);
// qap.hip: the witness map of device rows from the zkey's section 4 into d_h (arguments checked by the caller, the map built)
bool zkey_qap_enqueue(gwb_zkey* z, const void* d_witness, size_t batch, uint32_t form_in, void* d_h, uint32_t form_out, void* stream,
                      std::string& err);
// qap.hip: the device side of a zkey's witness map (arrays, tables, workspace)
void release_zkey_qap(gwb_zkey* z);
// qap.hip: the roots of the domain of 2^p points, Montgomery form: w_n of order n, g of order 2n with g^2 = w_n
void qap_roots(uint32_t p, cwc::Fr& wn, cwc::Fr& g);
// msm.hip: a uniform draw from [0, r), by rejection sampling from getrandom()
bool draw_fr(cwc::Fr& x, std::string& err);
}  // namespace cwc_r1cs
