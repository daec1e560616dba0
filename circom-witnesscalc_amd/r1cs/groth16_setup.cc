// groth16-setup [--trapdoor FILE] <circuit.r1cs> <circuit.zkey> [verification_key.json]: a Groth16 proving key for the
// circuit, made on the GPU (the single-party equivalent of snarkjs `groth16 setup`; include/graph_witness_groth16_setup.h).
// The trapdoor is drawn and discarded, or read from FILE: five decimal integers tau, alpha, beta, gamma, delta separated by
// whitespace, each in [1, r) (for reproducible keys).
// groth16-setup --ptau FILE [--delta FILE] [--lagrange auto|file|compute] <circuit.r1cs> <circuit.zkey> [verification_key.json]:
// the key from a powers-of-tau file, which is mapped into memory, not read (include/graph_witness_groth16_ptau.h): tau, alpha
// and beta are the ceremony's, gamma is 1, and delta is drawn and discarded or read from FILE (one decimal integer in [1, r);
// 1 gives the state of snarkjs `zkey new`).  --check-g2 (with --ptau only) first checks the G2 points the setup reads from
// the file for membership in the order-r subgroup, on the GPU, and refuses the file before a key is made if one is outside it.
// groth16-setup --prepare-ptau <in.ptau> <out.ptau>: what snarkjs `powersoftau prepare phase2` does (gwb_ptau_prepare_phase2): the
// input is mapped, the output is the input with its Lagrange sections 12 to 15 made on the GPU; nothing is printed on success.
// groth16-setup --check-lagrange [--domain-power P] <file.ptau>: checks sections 12 to 15 against 2 to 5 on the GPU
// (gwb_ptau_check_lagrange), the levels a setup for the domain 2^P reads or, without P, all of them; prints OK!, or exits with
// status 1 and the verdict.
// groth16-setup --export-vk <key.zkey> <verification_key.json>: the verifying key of any zkey in the same JSON shape (snarkjs `zkey
// export verificationkey`): after a contribution the key's delta has changed, and this writes the key that proofs are verified with.
// --ptau and --trapdoor exclude each other.  With a third path the verifying key is written too, in snarkjs's
// verification_key.json shape with vk_alphabeta_12.  Exit status 0 on success; 2 on a usage, file or format error.  Every
// input is parsed before the device is touched.
#include "../../include/graph_witness_groth16_compressed.h"
#include "../../include/graph_witness_groth16_ptau.h"
#include "../../include/graph_witness_groth16_setup.h"
#include "../../include/graph_witness_groth16_verify.h"
#include "cli_common.hpp"

using cli::decimal;
using R1cs = cli::Owned<gwb_r1cs_t, gwb_r1cs_free>;
using Zkey = cli::Owned<gwb_zkey_t, gwb_zkey_free>;
using Vk = cli::Owned<gwb_g16vk_t, gwb_g16vk_free>;
using Image = cli::Owned<void, gwb_groth16_setup_free>;  // a key or a file made by the library

// a file of `n` secrets, named in `names`, into le; false with the message printed: a wrong count before a bad value
static bool parse_secrets(const char* path, size_t n, const char* const* names, const char* all_names, uint8_t (*le)[32]) {
    cli::Secrets found;
    if (cli::parse_secret_decimals(path, n, le, found)) return true;
    if (!found.readable)
        cli::cannot_read(path);
    else if (found.tokens != n)
        fprintf(stderr, "error: %s: %zu values, %zu expected (%s)\n", path, found.tokens, n, all_names);
    else
        fprintf(stderr, "error: %s: %s is not a decimal integer below 2^256\n", path, names[found.bad]);
    return false;
}

static std::string g1_json(const uint8_t* p) {
    bool inf = true;
    for (int i = 0; i < 64; ++i) inf = inf && p[i] == 0;
    if (inf) return "[\"0\", \"1\", \"0\"]";
    return "[\"" + decimal(p) + "\", \"" + decimal(p + 32) + "\", \"1\"]";
}

static std::string g2_json(const uint8_t* p) {
    bool inf = true;
    for (int i = 0; i < 128; ++i) inf = inf && p[i] == 0;
    if (inf) return "[[\"0\", \"0\"], [\"1\", \"0\"], [\"0\", \"0\"]]";
    return "[[\"" + decimal(p) + "\", \"" + decimal(p + 32) + "\"], [\"" + decimal(p + 64) + "\", \"" + decimal(p + 96) + "\"], [\"1\", \"0\"]]";
}

// the verifying key of the written zkey as snarkjs's verification_key.json
static bool vk_json(const void* zkey, size_t len, std::string& out, std::string& err) {
    gw_status_t st = {OK, NULL};
    auto failed = [&](const char* what) {
        err = cli::take_message(st, what);
        return false;
    };
    gwb_zkey_t* z_loaded = NULL;
    if (gwb_zkey_load(zkey, len, &z_loaded, &st) != 0) return failed("loading the written key failed");
    const Zkey z(z_loaded);
    gwb_g16vk_t* vk_made = NULL;
    if (gwb_g16vk_from_zkey(z.get(), &vk_made, &st) != 0) return failed("extracting the verifying key failed");
    const Vk vk(vk_made);
    gwb_g16vk_info_t info;
    gwb_g16vk_info(vk.get(), &info);
    std::vector<uint8_t> pts(448 + 64 * ((size_t)info.n_public + 1));
    uint8_t gt[GWB_GT_BYTES];
    if (gwb_g16vk_points(vk.get(), pts.data(), pts.size()) != 0) return failed("reading the verifying key's points failed");
    if (gwb_g16vk_alphabeta(vk.get(), gt, &st) != 0) return failed("computing e(alpha1, beta2) failed");
    out = "{\n \"protocol\": \"groth16\",\n \"curve\": \"bn128\",\n \"nPublic\": " + std::to_string(info.n_public) + ",\n";
    out += " \"vk_alpha_1\": " + g1_json(pts.data()) + ",\n";
    out += " \"vk_beta_2\": " + g2_json(pts.data() + 64) + ",\n";
    out += " \"vk_gamma_2\": " + g2_json(pts.data() + 192) + ",\n";
    out += " \"vk_delta_2\": " + g2_json(pts.data() + 320) + ",\n";
    out += " \"vk_alphabeta_12\": [";
    for (int i = 0; i < 2; ++i) {
        out += i ? ", [" : "[";
        for (int j = 0; j < 3; ++j)
            out += std::string(j ? ", " : "") + "[\"" + decimal(gt + 32 * (6 * i + 2 * j)) + "\", \"" + decimal(gt + 32 * (6 * i + 2 * j + 1)) + "\"]";
        out += "]";
    }
    out += "],\n \"IC\": [";
    for (uint32_t i = 0; i <= info.n_public; ++i) out += std::string(i ? ",\n  " : "\n  ") + g1_json(pts.data() + 448 + 64 * (size_t)i);
    out += "\n ]\n}\n";
    return true;
}

static int usage_error(const char* argv0) {
    fprintf(stderr,
            "usage: %s [--trapdoor FILE] <circuit.r1cs> <circuit.zkey> [verification_key.json]\n"
            "       %s --ptau FILE [--delta FILE] [--lagrange auto|file|compute] [--check-g2] <circuit.r1cs> <circuit.zkey> [verification_key.json]\n"
            "       %s --prepare-ptau <in.ptau> <out.ptau>\n"
            "       %s --check-lagrange [--domain-power P] <file.ptau>\n"
            "       %s --export-vk <key.zkey> <verification_key.json>\n"
            "       %s --export-vk --compressed <key.zkey> <vk.bin>\n"
            "  --check-g2  refuse a file whose G2 points, as far as this setup reads them, are not all in the order-r subgroup\n"
            "  --prepare-ptau  write the file with its Lagrange sections 12 to 15 (snarkjs powersoftau prepare phase2)\n"
            "  --check-lagrange  check sections 12 to 15 against 2 to 5: the levels a setup for 2^P reads, or all of them\n"
            "  --export-vk  write the verifying key of any zkey, a finished ceremony's among them (snarkjs zkey export verificationkey)\n"
            "  --export-vk --compressed  write it as arkworks' compressed bytes, 232 + 32 (nPublic + 1)\n",
            argv0, argv0, argv0, argv0, argv0, argv0);
    return 2;
}

// --prepare-ptau and --check-lagrange: the file is mapped and parsed before the device is touched
static int ptau_tool(int argc, char** argv) {
    const bool prepare = strcmp(argv[1], "--prepare-ptau") == 0;
    uint32_t domain_power = GWB_PTAU_ALL_LEVELS;
    int at = 2;
    if (!prepare && argc > at + 1 && strcmp(argv[at], "--domain-power") == 0) {
        if (!cli::parse_u32(argv[at + 1], 28, domain_power)) return usage_error(argv[0]);
        at += 2;
    }
    if (argc - at != (prepare ? 2 : 1)) return usage_error(argv[0]);
    for (int i = at; i < argc; ++i)
        if (strncmp(argv[i], "--", 2) == 0) return usage_error(argv[0]);
    const char* path = argv[at];
    cli::Mapped in;
    if (!in.open(path)) return cli::cannot_read(path);
    gw_status_t st = {OK, NULL};  // both calls parse the file before they touch the device
    if (!prepare) {
        const int rc = gwb_ptau_check_lagrange(in.data, in.len, domain_power, NULL, &st);
        if (rc != 0) {
            cli::fail(path, st, "check failed");
            return rc == 1 ? 1 : 2;
        }
        printf("OK!\n");
        return 0;
    }
    void* out = NULL;
    size_t len = 0;
    if (gwb_ptau_prepare_phase2(in.data, in.len, &out, &len, &st) != 0) return cli::fail(path, st, "prepare failed");
    const Image image(out);
    return cli::write_file(argv[at + 1], out, len) ? 0 : cli::cannot_write(argv[at + 1]);
}

// --export-vk --compressed: the same key as arkworks' compressed bytes (include/graph_witness_groth16_compressed.h)
static int export_vk_compressed(char** argv) {
    std::vector<uint8_t> key, out;
    if (!cli::read_file(argv[3], key)) return cli::cannot_read(argv[3]);
    gw_status_t st = {OK, NULL};
    gwb_zkey_t* z_loaded = NULL;
    gwb_g16vk_t* vk_made = NULL;
    bool ok = gwb_zkey_load(key.data(), key.size(), &z_loaded, &st) == 0 && gwb_g16vk_from_zkey(z_loaded, &vk_made, &st) == 0;
    const Zkey z(z_loaded);
    const Vk vk(vk_made);
    if (ok) {
        gwb_g16vk_info_t info;
        gwb_g16vk_info(vk.get(), &info);
        out.resize(GWB_G16VK_COMPRESSED_BYTES(info.n_public));
        ok = gwb_g16vk_compressed(vk.get(), out.data(), out.size()) == 0;
    }
    if (!ok) return cli::fail(argv[3], st, "compressing the verifying key failed");
    return cli::write_file(argv[4], out.data(), out.size()) ? 0 : cli::cannot_write(argv[4]);
}

// --export-vk: the verifying key of any zkey, a finished ceremony's among them, as verification_key.json
static int export_vk(int argc, char** argv) {
    if (argc == 5 && strcmp(argv[2], "--compressed") == 0 && strncmp(argv[3], "--", 2) != 0 && strncmp(argv[4], "--", 2) != 0)
        return export_vk_compressed(argv);
    if (argc != 4 || strncmp(argv[2], "--", 2) == 0 || strncmp(argv[3], "--", 2) == 0) return usage_error(argv[0]);
    std::vector<uint8_t> key;
    if (!cli::read_file(argv[2], key)) return cli::cannot_read(argv[2]);
    std::string json, err;
    if (!vk_json(key.data(), key.size(), json, err)) {
        fprintf(stderr, "error: %s: %s\n", argv[2], err.c_str());
        return 2;
    }
    return cli::write_file(argv[3], json.data(), json.size()) ? 0 : cli::cannot_write(argv[3]);
}

int main(int argc, char** argv) {
    if (argc > 1 && (strcmp(argv[1], "--prepare-ptau") == 0 || strcmp(argv[1], "--check-lagrange") == 0)) return ptau_tool(argc, argv);
    if (argc > 1 && strcmp(argv[1], "--export-vk") == 0) return export_vk(argc, argv);
    const char *trapdoor_path = NULL, *ptau_path = NULL, *delta_path = NULL, *lagrange = NULL;
    std::vector<const char*> pos;
    bool usage = false, check_g2 = false;
    for (int i = 1; i < argc && !usage; ++i) {
        if (strcmp(argv[i], "--check-g2") == 0) {
            usage = check_g2;
            check_g2 = true;
            continue;
        }
        const char** opt = strcmp(argv[i], "--trapdoor") == 0 ? &trapdoor_path
                           : strcmp(argv[i], "--ptau") == 0   ? &ptau_path
                           : strcmp(argv[i], "--delta") == 0  ? &delta_path
                           : strcmp(argv[i], "--lagrange") == 0 ? &lagrange
                                                                : NULL;
        if (!opt)
            pos.push_back(argv[i]);
        else if (i + 1 >= argc || *opt)
            usage = true;
        else
            *opt = argv[++i];
    }
    uint32_t mode = GWB_PTAU_LAGRANGE_AUTO;
    if (lagrange) {
        if (strcmp(lagrange, "file") == 0)
            mode = GWB_PTAU_LAGRANGE_FILE;
        else if (strcmp(lagrange, "compute") == 0)
            mode = GWB_PTAU_LAGRANGE_COMPUTE;
        else if (strcmp(lagrange, "auto") != 0)
            usage = true;
    }
    // --ptau and --trapdoor exclude each other; --delta, --lagrange and --check-g2 belong to --ptau
    if ((ptau_path && trapdoor_path) || (!ptau_path && (delta_path || lagrange || check_g2))) usage = true;
    if (usage || (pos.size() != 2 && pos.size() != 3)) return usage_error(argv[0]);
    std::vector<uint8_t> file;
    if (!cli::read_file(pos[0], file)) return cli::cannot_read(pos[0]);
    gw_status_t st = {OK, NULL};
    gwb_r1cs_t* loaded = NULL;
    if (gwb_r1cs_load(file.data(), file.size(), &loaded, &st) != 0) return cli::fail(pos[0], st, "load failed");
    const R1cs r(loaded);
    static const char* const names[5] = {"tau", "alpha", "beta", "gamma", "delta"};
    uint8_t secrets[5][32] = {};  // the trapdoor, or delta in secrets[0]
    if (trapdoor_path && !parse_secrets(trapdoor_path, 5, names, "tau alpha beta gamma delta", secrets)) return 2;
    cli::Mapped ptau;
    if (ptau_path) {
        if (!ptau.open(ptau_path)) return cli::cannot_read(ptau_path);
        gwb_ptau_info_t pi;
        if (gwb_ptau_info(ptau.data, ptau.len, &pi, &st) != 0) return cli::fail(ptau_path, st, "load failed");
        if (delta_path && !parse_secrets(delta_path, 1, names + 4, "delta", secrets)) return 2;
    }
    void* zkey = NULL;
    size_t len = 0;
    int rc = 0;
    if (check_g2) {
        gwb_r1cs_qap_info_t qi;
        if (gwb_r1cs_qap_info(r.get(), &qi, &st) != 0 || gwb_ptau_check_g2(ptau.data, ptau.len, qi.domain_power, mode, &st) != 0)
            rc = cli::fail(ptau_path, st, "check failed");
    }
    if (rc == 0 && ptau_path) {
        fprintf(stderr,
                "groth16-setup: tau, alpha and beta are those of the ceremony behind %s, which is not verified here; single-party phase 2: "
                "whoever holds delta can forge proofs for this key; %s\n",
                ptau_path, delta_path ? "it was read from a file, which remains" : "a drawn delta is discarded before the key is written");
        if (gwb_groth16_setup_ptau(r.get(), ptau.data, ptau.len, delta_path ? secrets[0] : NULL, mode, &zkey, &len, &st) != 0) rc = cli::report(2, st, "setup failed");
    } else if (rc == 0) {
        fprintf(stderr, "groth16-setup: single-party setup: whoever holds the trapdoor can forge proofs for this key; %s\n",
                trapdoor_path ? "it was read from a file, which remains" : "a drawn trapdoor is discarded before the key is written");
        gwb_groth16_trapdoor_t t;
        static_assert(sizeof t == sizeof secrets, "the trapdoor is its five values in the order of the file");
        memcpy(&t, secrets, sizeof t);
        if (gwb_groth16_setup(r.get(), trapdoor_path ? &t : NULL, &zkey, &len, &st) != 0) rc = cli::report(2, st, "setup failed");
        explicit_bzero(&t, sizeof t);
    }
    explicit_bzero(secrets, sizeof secrets);
    if (rc != 0) return rc;
    const Image image(zkey);
    if (!cli::write_file(pos[1], zkey, len)) return cli::cannot_write(pos[1]);
    if (pos.size() == 3) {
        std::string json, err;
        if (!vk_json(zkey, len, json, err)) {
            fprintf(stderr, "error: %s\n", err.c_str());
            return 2;
        }
        if (!cli::write_file(pos[2], json.data(), json.size())) return cli::cannot_write(pos[2]);
    }
    return 0;
}
