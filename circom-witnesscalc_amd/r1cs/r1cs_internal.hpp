// Host representation of a loaded `.r1cs` file, shared by the loader (loader.cc), the device check (check.hip) and the QAP
// witness map (qap.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../csrc/fr_gfx950.hpp"
#include "../../include/graph_witness_r1cs.h"

namespace cwc_r1cs {

using cwc::Fr;

// Factor word: wire in the low 30 bits, kind in the top 2 bits.
constexpr uint32_t WIRE_MASK = 0x3fffffffu;
constexpr uint32_t KIND_GENERAL = 0u;  // coefficient coef[cidx] (Montgomery form c * R)
constexpr uint32_t KIND_PLUS = 1u;     // coefficient +1: the witness value is added
constexpr uint32_t KIND_MINUS = 2u;    // coefficient r - 1: the witness value is subtracted

// Constraint 0xFFFFFFFF is GWB_R1CS_SATISFIED, so indices stay below it.
constexpr uint64_t MAX_CONSTRAINTS = 0xfffffffeull;

void set_status(gw_status_t* st, const std::string& msg);
void set_ok(gw_status_t* st);

}  // namespace cwc_r1cs

struct gwb_r1cs;

// Host helpers of check.hip, shared with qap.hip.
namespace cwc_r1cs {
uint32_t pick_tile_width(size_t batch);                  // rows per wave for a batch
bool ensure_device(gwb_r1cs* r, std::string& err);       // constraint arrays on the current device (first call)
bool check_args(gwb_r1cs* r, size_t n_witness, size_t batch, std::string& err);
int fail(gw_status_t* st, const std::string& msg);      // set_status + return 1
// A `.wtns` image as gwb_r1cs_check_wtns validates it: the witness values (elements below r) and their count.
bool parse_wtns(const void* wtns, size_t len, const uint8_t** values, uint64_t* n_wit, std::string& err);

// Device state of one QAP domain (qap.hip), owned by the handle whose witness map runs on it (a gwb_r1cs, or a gwb_zkey
// proving from its section 4): twiddles w_n^e and per-position coset factors, n each, built at the first QAP call; the A / B
// workspace, grown on demand; phase-timing events (hipEvent_t, recorded around each phase while events[0] is set).
struct QapState {
    void *d_tw = nullptr, *d_coset = nullptr, *d_ws = nullptr;
    size_t ws_bytes = 0;
    void* events[5] = {};
};
void release_qap(QapState& q);                           // qap.hip: the QAP tables, workspace and events
}  // namespace cwc_r1cs

struct gwb_r1cs {
    gwb_r1cs_info_t info{};
    // Constraints in device order (bucketed by length, stable inside a bucket): constraint k's A factors are
    // fac[rowptr[3k] .. rowptr[3k+1]), B up to rowptr[3k+2], C up to rowptr[3k+3]; perm[k] = its index in the file.
    std::vector<uint32_t> rowptr, fac, cidx, perm;
    std::vector<cwc::Fr> coef;        // distinct general coefficients, Montgomery form
    std::vector<uint64_t> wire_label; // section 3 (kept for info, unused by the check)
    uint32_t tile_width = 0;          // 0 = from the batch size
    // device copies (first check call)
    int device = -1;
    void *d_rowptr = nullptr, *d_fac = nullptr, *d_cidx = nullptr, *d_coef = nullptr, *d_perm = nullptr;
    // QAP witness map (qap.hip, first QAP call, on the same device); its events are those of gwb_r1cs_qap_time_phases
    cwc_r1cs::QapState qap;
};
