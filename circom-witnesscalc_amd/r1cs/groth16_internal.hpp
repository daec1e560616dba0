// Host representation of a loaded `.zkey` (zkey.cc), shared with the prover (msm.hip) and the witness map (qap.hip), which
// evaluates the key's section 4 through the same row system as an `.r1cs` (r1cs_internal.hpp).
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
    cwc_r1cs::DeviceBuf d_a, d_b1, d_b2, d_c, d_h;
    cwc_r1cs::Workspace ws;
    cwc_r1cs::PinnedStage rs_stage;    // pinned staging of r, s
    cwc_r1cs::PhaseEvents<8> events;  // phase timing (gwb_groth16_time_phases): recorded around each phase of the last sub-batch
    // Section 4 as stored (n_coefs x 44 B: u32 matrix, constraint, signal, then the value c R^2 mod r), bounds-checked at load.
    std::vector<uint8_t> sec4;
    // The witness map of section 4 (zkey_coefs.cc, built at the first call that needs it): a row system without the C side, its
    // rows [0, n_rows) those up to the largest constraint index of any entry.  Its arrays go to the device of the points above,
    // if those are already there.
    bool coefs_built = false;
    cwc_r1cs::RowSystem sys;
    gwb_zkey() { sys.stride = 2; }
};

namespace cwc_r1cs {
// zkey_coefs.cc: builds the witness map of section 4 (first call; later calls return at once).  Refusals start "zkey:".
bool zkey_coefs_build(gwb_zkey* z, std::string& err);
// qap.hip: the witness map of device rows into d_h, as gwb_r1cs_qap_batch_device / gwb_zkey_qap_batch_device enqueue it: from
// the .r1cs, or from the zkey's section 4 (arguments checked by the caller, the map built)
bool qap_enqueue(gwb_r1cs* r, const void* d_witness, size_t batch, uint32_t form_in, void* d_h, uint32_t form_out, void* stream,
                 std::string& err);
bool qap_enqueue(gwb_zkey* z, const void* d_witness, size_t batch, uint32_t form_in, void* d_h, uint32_t form_out, void* stream,
                 std::string& err);
// qap.hip: the roots of the domain of 2^p points, Montgomery form: w_n of order n, g of order 2n with g^2 = w_n
void qap_roots(uint32_t p, cwc::Fr& wn, cwc::Fr& g);
// msm.hip: CWC_GROTH16_WORKSPACE_MB in bytes (4096 MB without it), read once per process: the prover's cap on a sub-batch's
// workspace, and the cap on the workspace of gwb_ptau_prepare_phase2 (setup_ptau.hip)
uint64_t groth16_workspace_cap();
// msm.hip: a uniform draw from [0, r), by rejection sampling from getrandom()
bool draw_fr(cwc::Fr& x, std::string& err);
}  // namespace cwc_r1cs
