// check-witness <circuit.r1cs> <witness.wtns>: does the witness satisfy every constraint of the circuit?  (snarkjs
// `wtns check`, on the GPU.)  Exit status 0: satisfied; 1: "constraint <j> not satisfied" (the smallest failing index);
// 2: usage, file or format error.
#include "../../include/graph_witness_r1cs.h"
#include "cli_common.hpp"

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <circuit.r1cs> <witness.wtns>\n", argv[0]);
        return 2;
    }
    std::vector<uint8_t> r1cs, wtns;
    for (int i = 1; i <= 2; ++i)
        if (!cli::read_file(argv[i], i == 1 ? r1cs : wtns)) return cli::cannot_read(argv[i]);
    gw_status_t st = {OK, NULL};
    gwb_r1cs_t* loaded = NULL;
    if (gwb_r1cs_load(r1cs.data(), r1cs.size(), &loaded, &st) != 0) return cli::fail(argv[1], st, "load failed");
    const cli::Owned<gwb_r1cs_t, gwb_r1cs_free> r(loaded);
    uint32_t first = 0, n_failed = 0;
    if (gwb_r1cs_check_wtns(r.get(), wtns.data(), wtns.size(), &first, &n_failed, &st) != 0) return cli::fail(argv[2], st, "check failed");
    if (first != GWB_R1CS_SATISFIED) {
        printf("constraint %u not satisfied (%u constraints fail)\n", first, n_failed);
        return 1;
    }
    printf("witness satisfies all constraints\n");
    return 0;
}
