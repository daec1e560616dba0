// groth16-prove <circuit.zkey> <witness.wtns> <proof.json> <public.json>: a Groth16 proof of the witness on the GPU (snarkjs
// `groth16 prove`, its argument order), written in snarkjs's proof.json / public.json shape; the witness map comes from the
// zkey's section 4.  groth16-prove <circuit.r1cs> <circuit.zkey> <witness.wtns> <proof.json> <public.json> takes it from the
// `.r1cs` instead.  --check-g2 (anywhere among the arguments, either form) first checks the key's G2 points (beta2, gamma2,
// delta2, section 7) for membership in the order-r subgroup, on the GPU, and refuses the key before proving if one is outside
// it.  Exit status 0 on success; 2 on a usage, file, format, mismatch or subgroup error.  Every input is parsed before the
// device is touched.  --compressed as the first argument writes the proof as the 128 raw bytes of arkworks' compressed form
// (include/graph_witness_groth16_compressed.h) in place of proof.json; public.json is unchanged.  (One proof's encoding is
// three comparisons: it is done here, with the host side of point_codec_gfx950.hpp.)
#include "../../include/graph_witness_groth16.h"
#include "cli_common.hpp"
#include "point_codec_gfx950.hpp"

using cli::decimal;

// the witness values of a `.wtns` image the library has already validated (section 2)
static const uint8_t* wtns_values(const std::vector<uint8_t>& w) {
    const uint8_t* p = w.data();
    uint32_t nsec;
    memcpy(&nsec, p + 8, 4);
    size_t off = 12;
    for (uint32_t i = 0; i < nsec; ++i) {
        uint32_t type;
        uint64_t size;
        memcpy(&type, p + off, 4);
        memcpy(&size, p + off + 4, 8);
        off += 12;
        if (type == 2) return p + off;
        off += size;
    }
    return nullptr;
}

int main(int argc, char** argv) {
    bool check_g2 = false, usage = false;
    const bool compressed = argc > 1 && strcmp(argv[1], "--compressed") == 0;
    std::vector<char*> pos;
    for (int i = compressed ? 2 : 1; i < argc; ++i) {
        if (strcmp(argv[i], "--check-g2") == 0) {
            usage = usage || check_g2;
            check_g2 = true;
        } else {
            pos.push_back(argv[i]);
        }
    }
    if (usage || (pos.size() != 4 && pos.size() != 5)) {
        fprintf(stderr,
                "usage: %s [--check-g2] <circuit.zkey> <witness.wtns> <proof.json> <public.json>\n"
                "       %s [--check-g2] <circuit.r1cs> <circuit.zkey> <witness.wtns> <proof.json> <public.json>\n"
                "  --check-g2  refuse a key whose G2 points are not all in the order-r subgroup (checked on the GPU before proving)\n"
                "  --compressed  as the first argument: write the proof as 128 raw bytes, arkworks' compressed form, in place of proof.json\n",
                argv[0], argv[0]);
        return 2;
    }
    const bool with_r1cs = pos.size() == 5;
    char** in = pos.data();  // inputs: [r1cs,] zkey, wtns; then the two outputs
    const int n_in = with_r1cs ? 3 : 2;
    std::vector<uint8_t> loaded[3];
    for (int i = 0; i < n_in; ++i)
        if (!cli::read_file(in[i], loaded[i])) return cli::cannot_read(in[i]);
    const std::vector<uint8_t>& zkey_file = loaded[n_in - 2];
    const std::vector<uint8_t>& wtns_file = loaded[n_in - 1];
    gw_status_t st = {OK, NULL};
    gwb_r1cs_t* r_loaded = NULL;
    gwb_zkey_t* z_loaded = NULL;
    if (with_r1cs && gwb_r1cs_load(loaded[0].data(), loaded[0].size(), &r_loaded, &st) != 0) return cli::fail(in[0], st, "load failed");
    const cli::Owned<gwb_r1cs_t, gwb_r1cs_free> r(r_loaded);
    if (gwb_zkey_load(zkey_file.data(), zkey_file.size(), &z_loaded, &st) != 0) return cli::fail(in[n_in - 2], st, "load failed");
    const cli::Owned<gwb_zkey_t, gwb_zkey_free> z(z_loaded);
    if (check_g2) {  // the witness is parsed first, so that the subgroup check is not the first to find a broken image
        const bool parsed = gwb_zkey_check_wtns(z.get(), wtns_file.data(), wtns_file.size(), &st) == 0;
        if (!parsed || gwb_zkey_check_g2(z.get(), &st) != 0) return cli::fail(in[parsed ? n_in - 2 : n_in - 1], st, "check failed");
    }
    uint8_t proof[GWB_GROTH16_PROOF_BYTES];
    // (the call parses the .wtns image and, without an .r1cs, builds the map of section 4 before it reaches the device)
    if (gwb_groth16_prove_wtns(z.get(), r.get(), wtns_file.data(), wtns_file.size(), NULL, proof, &st) != 0) return cli::fail(in[n_in - 1], st, "prove failed");
    gwb_zkey_info_t zi;
    gwb_zkey_info(z.get(), &zi);
    auto d = [&](int k) { return "\"" + decimal(proof + 32 * k) + "\""; };
    // snarkjs writes projective coordinates with z = 1 (or 0 for the point at infinity)
    auto z1 = [&](int k, int words) {
        for (int i = 0; i < words * 32; ++i)
            if (proof[32 * k + i]) return std::string("\"1\"");
        return std::string("\"0\"");
    };
    std::string pj = "{\n \"pi_a\": [\n  " + d(0) + ",\n  " + d(1) + ",\n  " + z1(0, 2) + "\n ],\n \"pi_b\": [\n  [\n   " + d(2) + ",\n   " + d(3) +
                     "\n  ],\n  [\n   " + d(4) + ",\n   " + d(5) + "\n  ],\n  [\n   " + z1(2, 4) + ",\n   \"0\"\n  ]\n ],\n \"pi_c\": [\n  " + d(6) +
                     ",\n  " + d(7) + ",\n  " + z1(6, 2) + "\n ],\n \"protocol\": \"groth16\",\n \"curve\": \"bn128\"\n}\n";
    if (compressed) {
        uint8_t c[128];
        cwc_g16::g1_encode(proof, true, c);
        cwc_g16::g2_encode(proof + 64, true, c + 32);
        cwc_g16::g1_encode(proof + 192, true, c + 96);
        pj.assign((const char*)c, sizeof c);
    }
    const uint8_t* w = wtns_values(wtns_file);
    std::string pub = "[";
    for (uint32_t i = 1; i <= zi.n_public; ++i) pub += std::string(i > 1 ? ",\n " : "\n ") + "\"" + decimal(w + 32 * (size_t)i) + "\"";
    pub += zi.n_public ? "\n]\n" : "]\n";
    if (!cli::write_file(in[n_in], pj.data(), pj.size()) || !cli::write_file(in[n_in + 1], pub.data(), pub.size())) {
        fprintf(stderr, "error: cannot write %s / %s\n", in[n_in], in[n_in + 1]);
        return 2;
    }
    return 0;
}
