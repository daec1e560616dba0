// Host-only check that the graph compiler sees the environment through its caller's snapshot alone (csrc/knobs.hpp): built with
// -fsanitize=address,undefined by tests/test_knobs_snapshot_host.py, no HIP.  A snapshot is taken with CWC_NO_BIT_SCANS set, the
// variable is removed, and a worker thread compiles a wide-register long-division graph with its copy of the snapshot: the
// program must hold no borrow / comparison / selection bundles.  Then the reverse: snapshot with the variable unset, variable
// set, compile on a worker: the bundles must be there.  Exit code 0 and "OK" = both held.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <thread>

#include "../../circom-witnesscalc_amd/csrc/program.hpp"
#include "../../include/graph_witness_batch.h"

using namespace cwc;

// bundles of one-bit recurrences in a program (a selection bundle carries both bits)
static void bit_scan_bundles(const Program& p, unsigned& borrow, unsigned& lex) {
    borrow = lex = 0;
    for (uint32_t h : p.hdr)
        if ((h & HDR_CLASS_MASK) == C_SCAN) {
            borrow += (h & HDR_SCAN_BORROW) != 0;
            lex += (h & HDR_SCAN_LEX) != 0;
        }
}

// compiles on a thread of its own, which holds a copy of the snapshot
static bool compile_on_worker(const Graph& g, const Knobs& snapshot, uint32_t T, Program& p, std::string& err) {
    bool ok = false;
    std::thread worker([&g, k = snapshot, T, &p, &err, &ok]() { ok = compile_program(g, k, T, 0, p, err); });
    worker.join();
    return ok;
}

int main() {
    void* bin = nullptr;
    size_t bin_len = 0;
    gw_status_t st{OK, nullptr};
    if (gwb_graphgen_rsa_long_div_class(64, 4, 1, 0, &bin, &bin_len, &st) != 0) {
        printf("generator failed: %s\n", st.error_msg ? st.error_msg : "?");
        return 1;
    }
    Graph g;
    std::string err;
    const bool parsed = deserialize_witnesscalc_graph((const uint8_t*)bin, bin_len, g, err);
    free(bin);
    if (!parsed) {
        printf("generated graph rejected: %s\n", err.c_str());
        return 1;
    }
    int rc = 0;
    for (uint32_t T : {1u, 2u}) {
        unsigned nb = 0, nl = 0;
        Program p;
        // the snapshot says "no bit scans", the environment at compile time says nothing
        setenv("CWC_NO_BIT_SCANS", "1", 1);
        const Knobs off = read_knobs();
        unsetenv("CWC_NO_BIT_SCANS");
        if (!compile_on_worker(g, off, T, p, err)) {
            printf("T=%u: compile failed: %s\n", T, err.c_str());
            return 1;
        }
        bit_scan_bundles(p, nb, nl);
        if (!off.no_bit_scans || nb != 0 || nl != 0) {
            printf("T=%u: snapshot with CWC_NO_BIT_SCANS, variable removed: %u borrow and %u comparison bundles, want none\n", T, nb, nl);
            rc = 1;
        }
        // the snapshot says nothing, the environment at compile time says "no bit scans"
        const Knobs on = read_knobs();
        setenv("CWC_NO_BIT_SCANS", "1", 1);
        p = Program();
        if (!compile_on_worker(g, on, T, p, err)) {
            printf("T=%u: compile failed: %s\n", T, err.c_str());
            return 1;
        }
        unsetenv("CWC_NO_BIT_SCANS");
        bit_scan_bundles(p, nb, nl);
        if (on.no_bit_scans || nb == 0 || nl == 0) {
            printf("T=%u: snapshot without CWC_NO_BIT_SCANS, variable set: %u borrow and %u comparison bundles, want both kinds\n", T, nb, nl);
            rc = 1;
        }
    }
    printf(rc ? "FAILED\n" : "OK\n");
    return rc;
}
