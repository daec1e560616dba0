// Host representation of a loaded `.r1cs` file, shared by the loader (loader.cc), the device check (check.hip) and the QAP
// witness map (qap.hip), and the row system both it and a zkey's section 4 (groth16_internal.hpp) are evaluated through.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../csrc/fr_gfx950.hpp"
#include "device_owners.hpp"
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

// Host helpers of check.hip, shared with qap.hip and msm.hip.
namespace cwc_r1cs {
int fail(gw_status_t* st, const std::string& msg);      // set_status + return 1
// A `.wtns` image as gwb_r1cs_check_wtns validates it: the witness values (elements below r) and their count.
bool parse_wtns(const void* wtns, size_t len, const uint8_t** values, uint64_t* n_wit, std::string& err);

// Device state of one QAP domain (qap.hip), owned by the row system whose witness map runs on it: twiddles w_n^e and
// per-position coset factors, n each, built at the first QAP call; the A / B workspace, grown on demand; phase-timing events
// (recorded around each phase while timing is on).
struct QapState {
    DeviceBuf tw, coset;
    Workspace ws;
    PhaseEvents<5> events;
};

// Rows of linear combinations over a witness, as the check and evaluation kernels read them (lincomb.hpp): an `.r1cs`
// (loader.cc; stride 3: sides A, B, C) or section 4 of a zkey (zkey_coefs.cc; stride 2: A, B, the public rows among them).
// Rows are in device order (bucketed by length, stable inside a bucket): side m of row k is fac[rowptr[stride k + m] ..
// rowptr[stride k + m + 1]), and perm[k] is the row's constraint index.  The stride also tells the two sources apart where
// they differ: the prefix of a refusal ("r1cs: " / "zkey: ") and the kernel that fills the rows above n_rows (qap.hip).
struct RowSystem {
    std::vector<uint32_t> rowptr, fac, cidx, perm;
    std::vector<cwc::Fr> coef;  // distinct general coefficients, Montgomery form c R
    uint32_t stride = 3;        // row pointers per row
    uint32_t n_rows = 0;        // evaluated rows: n_constraints, or 1 + the largest constraint index of section 4
    uint32_t n_wires = 0;       // elements per witness row: n_wires, or nVars
    uint32_t tile_width = 0;    // witness rows per wave, 0 = from the batch size
    // device copies (first call that needs them; all five or none) and the QAP domain's state, on the same device
    int device = -1;
    DeviceBuf d_rowptr, d_fac, d_cidx, d_coef, d_perm;
    QapState qap;
};

const char* prefix_of(const RowSystem& s);               // "r1cs: " or "zkey: "
// The arrays go to the current device at the first call and stay there; `home` >= 0 names the device they have to share
// (a zkey's uploaded points), -1 leaves the choice to the current device.
bool ensure_device(RowSystem& s, int home, std::string& err);
bool check_args(const RowSystem& s, size_t n_witness, size_t batch, std::string& err);

// Grid of a kernel with the check's lane mapping: a wave covers t rows x 64 / t constraints, blockIdx.x walks the `tiles`
// groups of t rows, and gy blocks of `waves` waves stride over the constraint groups: about eight blocks per CU in all.
struct EvalGrid {
    uint32_t t, tiles, gy;
};
int cu_count(int device);                                // 256 where the device does not say
bool eval_grid(const RowSystem& s, uint64_t rows, int cus, int waves, EvalGrid& g, std::string& err);
}  // namespace cwc_r1cs

struct gwb_r1cs {
    gwb_r1cs_info_t info{};
    cwc_r1cs::RowSystem sys;          // the constraints, stride 3; the QAP events are those of gwb_r1cs_qap_time_phases
    std::vector<uint64_t> wire_label; // section 3 (kept for info, unused by the check)
};
