// check-witness <circuit.r1cs> <witness.wtns>: does the witness satisfy every constraint of the circuit?  (snarkjs
// `wtns check`, on the GPU.)  Exit status 0: satisfied; 1: "constraint <j> not satisfied" (the smallest failing index);
// 2: usage, file or format error.
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iterator>
#include <vector>

#include "../../include/graph_witness_r1cs.h"

static bool read_file(const char* path, std::vector<char>& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return !f.bad();
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <circuit.r1cs> <witness.wtns>\n", argv[0]);
        return 2;
    }
    std::vector<char> r1cs, wtns;
    for (int i = 1; i <= 2; ++i) {
        if (!read_file(argv[i], i == 1 ? r1cs : wtns)) {
            fprintf(stderr, "error: cannot read %s\n", argv[i]);
            return 2;
        }
    }
    gw_status_t st = {OK, NULL};
    gwb_r1cs_t* r = NULL;
    if (gwb_r1cs_load(r1cs.data(), r1cs.size(), &r, &st) != 0) {
        fprintf(stderr, "error: %s: %s\n", argv[1], st.error_msg ? st.error_msg : "load failed");
        gw_free_status(&st);
        return 2;
    }
    uint32_t first = 0, n_failed = 0;
    const int rc = gwb_r1cs_check_wtns(r, wtns.data(), wtns.size(), &first, &n_failed, &st);
    gwb_r1cs_free(r);
    if (rc != 0) {
        fprintf(stderr, "error: %s: %s\n", argv[2], st.error_msg ? st.error_msg : "check failed");
        gw_free_status(&st);
        return 2;
    }
    if (first != GWB_R1CS_SATISFIED) {
        printf("constraint %u not satisfied (%u constraints fail)\n", first, n_failed);
        return 1;
    }
    printf("witness satisfies all constraints\n");
    return 0;
}
