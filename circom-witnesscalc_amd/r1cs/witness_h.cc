// witness-h <circuit.r1cs> <witness.wtns> <out.bin>: the Groth16 witness map of one witness on the GPU (what snarkjs
// `groth16 prove` computes before its H-point MSM): writes the n canonical 32-byte little-endian elements of h
// (include/graph_witness_r1cs.h has the definition).  Exit status 0: written; 2: usage, file or format error.
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
    if (argc != 4) {
        fprintf(stderr, "usage: %s <circuit.r1cs> <witness.wtns> <out.bin>\n", argv[0]);
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
    gwb_r1cs_qap_info_t info;
    if (gwb_r1cs_qap_info(r, &info, &st) != 0) {
        fprintf(stderr, "error: %s: %s\n", argv[1], st.error_msg ? st.error_msg : "no QAP domain");
        gw_free_status(&st);
        gwb_r1cs_free(r);
        return 2;
    }
    std::vector<unsigned char> h(info.domain_size * 32);
    const int rc = gwb_r1cs_qap_wtns(r, wtns.data(), wtns.size(), h.data(), GWB_FORM_CANONICAL, &st);
    gwb_r1cs_free(r);
    if (rc != 0) {
        fprintf(stderr, "error: %s: %s\n", argv[2], st.error_msg ? st.error_msg : "witness map failed");
        gw_free_status(&st);
        return 2;
    }
    FILE* f = fopen(argv[3], "wb");
    if (!f || fwrite(h.data(), 1, h.size(), f) != h.size() || fclose(f) != 0) {
        fprintf(stderr, "error: cannot write %s\n", argv[3]);
        return 2;
    }
    printf("h: %llu elements (domain 2^%u) written to %s\n", (unsigned long long)info.domain_size, info.domain_power, argv[3]);
    return 0;
}
