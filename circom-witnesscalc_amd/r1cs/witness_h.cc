// witness-h <circuit.r1cs> <witness.wtns> <out.bin>: the Groth16 witness map of one witness on the GPU (what snarkjs
// `groth16 prove` computes before its H-point MSM): writes the n canonical 32-byte little-endian elements of h
// (include/graph_witness_r1cs.h has the definition).  Exit status 0: written; 2: usage, file or format error.
#include "../../include/graph_witness_r1cs.h"
#include "cli_common.hpp"

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s <circuit.r1cs> <witness.wtns> <out.bin>\n", argv[0]);
        return 2;
    }
    std::vector<uint8_t> r1cs, wtns;
    for (int i = 1; i <= 2; ++i)
        if (!cli::read_file(argv[i], i == 1 ? r1cs : wtns)) return cli::cannot_read(argv[i]);
    gw_status_t st = {OK, NULL};
    gwb_r1cs_t* loaded = NULL;
    if (gwb_r1cs_load(r1cs.data(), r1cs.size(), &loaded, &st) != 0) return cli::fail(argv[1], st, "load failed");
    const cli::Owned<gwb_r1cs_t, gwb_r1cs_free> r(loaded);
    gwb_r1cs_qap_info_t info;
    if (gwb_r1cs_qap_info(r.get(), &info, &st) != 0) return cli::fail(argv[1], st, "no QAP domain");
    std::vector<unsigned char> h(info.domain_size * 32);
    if (gwb_r1cs_qap_wtns(r.get(), wtns.data(), wtns.size(), h.data(), GWB_FORM_CANONICAL, &st) != 0) return cli::fail(argv[2], st, "witness map failed");
    if (!cli::write_file(argv[3], h.data(), h.size())) return cli::cannot_write(argv[3]);
    printf("h: %llu elements (domain 2^%u) written to %s\n", (unsigned long long)info.domain_size, info.domain_power, argv[3]);
    return 0;
}
