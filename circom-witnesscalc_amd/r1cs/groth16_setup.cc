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
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/graph_witness_groth16_compressed.h"
#include "../../include/graph_witness_groth16_ptau.h"
#include "../../include/graph_witness_groth16_setup.h"
#include "../../include/graph_witness_groth16_verify.h"

static bool read_file(const char* path, std::vector<char>& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return !f.bad();
}

static bool write_file(const char* path, const void* data, size_t n) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(data, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

// 32-byte little-endian integer -> decimal string
static std::string decimal(const uint8_t* le) {
    uint32_t w[8];
    memcpy(w, le, 32);
    std::string out;
    for (;;) {
        bool zero = true;
        uint64_t rem = 0;
        for (int i = 7; i >= 0; --i) {
            const uint64_t cur = (rem << 32) | w[i];
            w[i] = (uint32_t)(cur / 1000000000u);
            rem = cur % 1000000000u;
            zero = zero && w[i] == 0;
        }
        char buf[16];
        snprintf(buf, sizeof buf, zero ? "%llu" : "%09llu", (unsigned long long)rem);
        out = buf + out;
        if (zero) return out;
    }
}

// decimal digits -> 32-byte little-endian integer; false for another character, no digit, or a value of 2^256 or more
static bool parse_decimal(const std::string& tok, uint8_t* le) {
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (tok.empty()) return false;
    for (char c : tok) {
        if (c < '0' || c > '9') return false;
        uint64_t carry = (uint64_t)(c - '0');
        for (int i = 0; i < 8; ++i) {
            const uint64_t cur = (uint64_t)w[i] * 10 + carry;
            w[i] = (uint32_t)cur;
            carry = cur >> 32;
        }
        if (carry) return false;
    }
    memcpy(le, w, 32);
    return true;
}

// the whitespace-separated tokens of a file of secrets; the file's text is zeroed
static bool read_tokens(const char* path, std::vector<std::string>& toks) {
    std::vector<char> text;
    if (!read_file(path, text)) {
        fprintf(stderr, "error: cannot read %s\n", path);
        return false;
    }
    std::string cur;
    for (char c : text) {
        if (c == ' ' || c == '\n' || c == '\r' || c == '\t') {
            if (!cur.empty()) toks.push_back(cur);
            cur.clear();
        } else {
            cur += c;
        }
    }
    if (!cur.empty()) toks.push_back(cur);
    std::fill(text.begin(), text.end(), 0);
    return true;
}

static bool parse_trapdoor(const char* path, gwb_groth16_trapdoor_t* t) {
    std::vector<std::string> toks;
    if (!read_tokens(path, toks)) return false;
    if (toks.size() != 5) {
        fprintf(stderr, "error: %s: %zu values, 5 expected (tau alpha beta gamma delta)\n", path, toks.size());
        return false;
    }
    static const char* names[5] = {"tau", "alpha", "beta", "gamma", "delta"};
    uint8_t* dst[5] = {t->tau, t->alpha, t->beta, t->gamma, t->delta};
    for (int i = 0; i < 5; ++i)
        if (!parse_decimal(toks[i], dst[i])) {
            fprintf(stderr, "error: %s: %s is not a decimal integer below 2^256\n", path, names[i]);
            return false;
        }
    return true;
}

static bool parse_delta(const char* path, uint8_t* delta) {
    std::vector<std::string> toks;
    if (!read_tokens(path, toks)) return false;
    if (toks.size() != 1) {
        fprintf(stderr, "error: %s: %zu values, 1 expected (delta)\n", path, toks.size());
        return false;
    }
    if (!parse_decimal(toks[0], delta)) {
        fprintf(stderr, "error: %s: delta is not a decimal integer below 2^256\n", path);
        return false;
    }
    return true;
}

// a file mapped read-only; size 0 maps nothing
struct Mapped {
    void* data = NULL;
    size_t len = 0;
    bool open(const char* path) {
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        bool ok = fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
        if (ok && st.st_size > 0) {
            void* p = mmap(NULL, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            ok = p != MAP_FAILED;
            if (ok) {
                data = p;
                len = (size_t)st.st_size;
            }
        }
        close(fd);
        return ok;
    }
    ~Mapped() {
        if (data) munmap(data, len);
    }
};

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
    gwb_zkey_t* z = NULL;
    gwb_g16vk_t* vk = NULL;
    auto failed = [&](const char* what) {
        err = st.error_msg ? st.error_msg : what;
        gw_free_status(&st);
        if (vk) gwb_g16vk_free(vk);
        if (z) gwb_zkey_free(z);
        return false;
    };
    if (gwb_zkey_load(zkey, len, &z, &st) != 0) return failed("loading the written key failed");
    if (gwb_g16vk_from_zkey(z, &vk, &st) != 0) return failed("extracting the verifying key failed");
    gwb_g16vk_info_t info;
    gwb_g16vk_info(vk, &info);
    std::vector<uint8_t> pts(448 + 64 * ((size_t)info.n_public + 1));
    uint8_t gt[GWB_GT_BYTES];
    if (gwb_g16vk_points(vk, pts.data(), pts.size()) != 0) return failed("reading the verifying key's points failed");
    if (gwb_g16vk_alphabeta(vk, gt, &st) != 0) return failed("computing e(alpha1, beta2) failed");
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
    gwb_g16vk_free(vk);
    gwb_zkey_free(z);
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
        char* end = NULL;
        const unsigned long v = strtoul(argv[at + 1], &end, 10);
        if (!*argv[at + 1] || *end || v > 28) return usage_error(argv[0]);
        domain_power = (uint32_t)v;
        at += 2;
    }
    if (argc - at != (prepare ? 2 : 1)) return usage_error(argv[0]);
    for (int i = at; i < argc; ++i)
        if (strncmp(argv[i], "--", 2) == 0) return usage_error(argv[0]);
    const char* path = argv[at];
    Mapped in;
    if (!in.open(path)) {
        fprintf(stderr, "error: cannot read %s\n", path);
        return 2;
    }
    gw_status_t st = {OK, NULL};  // both calls parse the file before they touch the device
    if (!prepare) {
        const int rc = gwb_ptau_check_lagrange(in.data, in.len, domain_power, NULL, &st);
        if (rc != 0) {
            fprintf(stderr, "error: %s: %s\n", path, st.error_msg ? st.error_msg : "check failed");
            gw_free_status(&st);
            return rc == 1 ? 1 : 2;
        }
        printf("OK!\n");
        return 0;
    }
    void* out = NULL;
    size_t len = 0;
    if (gwb_ptau_prepare_phase2(in.data, in.len, &out, &len, &st) != 0) {
        fprintf(stderr, "error: %s: %s\n", path, st.error_msg ? st.error_msg : "prepare failed");
        gw_free_status(&st);
        return 2;
    }
    int code = 0;
    if (!write_file(argv[at + 1], out, len)) {
        fprintf(stderr, "error: cannot write %s\n", argv[at + 1]);
        code = 2;
    }
    gwb_groth16_setup_free(out);
    return code;
}

// --export-vk --compressed: the same key as arkworks' compressed bytes (include/graph_witness_groth16_compressed.h)
static int export_vk_compressed(char** argv) {
    std::vector<char> key;
    if (!read_file(argv[3], key)) {
        fprintf(stderr, "error: cannot read %s\n", argv[3]);
        return 2;
    }
    gw_status_t st = {OK, NULL};
    gwb_zkey_t* z = NULL;
    gwb_g16vk_t* vk = NULL;
    std::vector<uint8_t> out;
    bool ok = gwb_zkey_load(key.data(), key.size(), &z, &st) == 0 && gwb_g16vk_from_zkey(z, &vk, &st) == 0;
    if (ok) {
        gwb_g16vk_info_t info;
        gwb_g16vk_info(vk, &info);
        out.resize(GWB_G16VK_COMPRESSED_BYTES(info.n_public));
        ok = gwb_g16vk_compressed(vk, out.data(), out.size()) == 0;
    }
    if (vk) gwb_g16vk_free(vk);
    if (z) gwb_zkey_free(z);
    if (!ok) {
        fprintf(stderr, "error: %s: %s\n", argv[3], st.error_msg ? st.error_msg : "compressing the verifying key failed");
        gw_free_status(&st);
        return 2;
    }
    if (!write_file(argv[4], out.data(), out.size())) {
        fprintf(stderr, "error: cannot write %s\n", argv[4]);
        return 2;
    }
    return 0;
}

// --export-vk: the verifying key of any zkey, a finished ceremony's among them, as verification_key.json
static int export_vk(int argc, char** argv) {
    if (argc == 5 && strcmp(argv[2], "--compressed") == 0 && strncmp(argv[3], "--", 2) != 0 && strncmp(argv[4], "--", 2) != 0)
        return export_vk_compressed(argv);
    if (argc != 4 || strncmp(argv[2], "--", 2) == 0 || strncmp(argv[3], "--", 2) == 0) return usage_error(argv[0]);
    std::vector<char> key;
    if (!read_file(argv[2], key)) {
        fprintf(stderr, "error: cannot read %s\n", argv[2]);
        return 2;
    }
    std::string json, err;
    if (!vk_json(key.data(), key.size(), json, err)) {
        fprintf(stderr, "error: %s: %s\n", argv[2], err.c_str());
        return 2;
    }
    if (!write_file(argv[3], json.data(), json.size())) {
        fprintf(stderr, "error: cannot write %s\n", argv[3]);
        return 2;
    }
    return 0;
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
    std::vector<char> file;
    if (!read_file(pos[0], file)) {
        fprintf(stderr, "error: cannot read %s\n", pos[0]);
        return 2;
    }
    gw_status_t st = {OK, NULL};
    gwb_r1cs_t* r = NULL;
    if (gwb_r1cs_load(file.data(), file.size(), &r, &st) != 0) {
        fprintf(stderr, "error: %s: %s\n", pos[0], st.error_msg ? st.error_msg : "load failed");
        gw_free_status(&st);
        return 2;
    }
    gwb_groth16_trapdoor_t t;
    if (trapdoor_path && !parse_trapdoor(trapdoor_path, &t)) {
        gwb_r1cs_free(r);
        return 2;
    }
    Mapped ptau;
    uint8_t delta[32];
    if (ptau_path) {
        if (!ptau.open(ptau_path)) {
            fprintf(stderr, "error: cannot read %s\n", ptau_path);
            gwb_r1cs_free(r);
            return 2;
        }
        gwb_ptau_info_t pi;
        if (gwb_ptau_info(ptau.data, ptau.len, &pi, &st) != 0) {
            fprintf(stderr, "error: %s: %s\n", ptau_path, st.error_msg ? st.error_msg : "load failed");
            gw_free_status(&st);
            gwb_r1cs_free(r);
            return 2;
        }
        if (delta_path && !parse_delta(delta_path, delta)) {
            gwb_r1cs_free(r);
            return 2;
        }
    }
    if (check_g2) {
        gwb_r1cs_qap_info_t qi;
        if (gwb_r1cs_qap_info(r, &qi, &st) != 0 || gwb_ptau_check_g2(ptau.data, ptau.len, qi.domain_power, mode, &st) != 0) {
            fprintf(stderr, "error: %s: %s\n", ptau_path, st.error_msg ? st.error_msg : "check failed");
            gw_free_status(&st);
            explicit_bzero(delta, sizeof delta);
            gwb_r1cs_free(r);
            return 2;
        }
    }
    void* zkey = NULL;
    size_t len = 0;
    int rc;
    if (ptau_path) {
        fprintf(stderr,
                "groth16-setup: tau, alpha and beta are those of the ceremony behind %s, which is not verified here; single-party phase 2: "
                "whoever holds delta can forge proofs for this key; %s\n",
                ptau_path, delta_path ? "it was read from a file, which remains" : "a drawn delta is discarded before the key is written");
        rc = gwb_groth16_setup_ptau(r, ptau.data, ptau.len, delta_path ? delta : NULL, mode, &zkey, &len, &st);
        explicit_bzero(delta, sizeof delta);
    } else {
        fprintf(stderr, "groth16-setup: single-party setup: whoever holds the trapdoor can forge proofs for this key; %s\n",
                trapdoor_path ? "it was read from a file, which remains" : "a drawn trapdoor is discarded before the key is written");
        rc = gwb_groth16_setup(r, trapdoor_path ? &t : NULL, &zkey, &len, &st);
    }
    explicit_bzero(&t, sizeof t);
    gwb_r1cs_free(r);
    if (rc != 0) {
        fprintf(stderr, "error: %s\n", st.error_msg ? st.error_msg : "setup failed");
        gw_free_status(&st);
        return 2;
    }
    int code = 0;
    if (!write_file(pos[1], zkey, len)) {
        fprintf(stderr, "error: cannot write %s\n", pos[1]);
        code = 2;
    }
    if (code == 0 && pos.size() == 3) {
        std::string json, err;
        if (!vk_json(zkey, len, json, err)) {
            fprintf(stderr, "error: %s\n", err.c_str());
            code = 2;
        } else if (!write_file(pos[2], json.data(), json.size())) {
            fprintf(stderr, "error: cannot write %s\n", pos[2]);
            code = 2;
        }
    }
    gwb_groth16_setup_free(zkey);
    return code;
}
