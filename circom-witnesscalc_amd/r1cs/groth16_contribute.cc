// groth16-contribute [--name NAME] [--delta FILE] <in.zkey> <out.zkey>: one phase-2 contribution to a Groth16 key, made on the
// GPU (include/graph_witness_groth16_contribute.h).  The secret is drawn and discarded, or read from FILE (one decimal integer
// in [1, r), for reproducible keys).  Prints the contribution hash in hex.
// groth16-contribute --verify <key.zkey>: checks the key's contribution records and prints their hashes.
// groth16-contribute --verify-step <prev.zkey> <next.zkey>: checks that next is prev after exactly one contribution.
// The records are this library's own: they are not interchangeable with snarkjs's (see the header).  Exit status 0 on success;
// 1 for a failed verification, with its message; 2 on a usage, file or format error.  Every input is parsed before the device
// is touched.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/graph_witness_groth16_contribute.h"
#include "../../include/graph_witness_groth16_setup.h"

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

// a file with one decimal integer below 2^256 -> 32 little-endian bytes; the file's text is zeroed
static bool parse_delta(const char* path, uint8_t* le) {
    std::vector<char> text;
    if (!read_file(path, text)) {
        fprintf(stderr, "error: cannot read %s\n", path);
        return false;
    }
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    size_t digits = 0, tokens = 0;
    bool ok = true, in_token = false;
    for (char c : text) {
        if (c == ' ' || c == '\n' || c == '\r' || c == '\t') {
            in_token = false;
            continue;
        }
        if (!in_token) ++tokens;
        in_token = true;
        if (c < '0' || c > '9') {
            ok = false;
            break;
        }
        ++digits;
        uint64_t carry = (uint64_t)(c - '0');
        for (int i = 0; i < 8; ++i) {
            const uint64_t cur = (uint64_t)w[i] * 10 + carry;
            w[i] = (uint32_t)cur;
            carry = cur >> 32;
        }
        if (carry) ok = false;
    }
    std::fill(text.begin(), text.end(), 0);
    if (!ok || digits == 0 || tokens != 1) {
        fprintf(stderr, "error: %s: one decimal integer below 2^256 expected (delta)\n", path);
        return false;
    }
    memcpy(le, w, 32);
    return true;
}

static void print_hex(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
    printf("\n");
}

static int usage() {
    fprintf(stderr,
            "usage: groth16-contribute [--name NAME] [--delta FILE] <in.zkey> <out.zkey>\n"
            "       groth16-contribute --verify <key.zkey>\n"
            "       groth16-contribute --verify-step <prev.zkey> <next.zkey>\n");
    return 2;
}

static int report(int rc, gw_status_t& st) {
    fprintf(stderr, "%s: %s\n", rc == 1 ? "INVALID" : "error", st.error_msg ? st.error_msg : "call failed");
    free(st.error_msg);
    return rc == 1 ? 1 : 2;
}

int main(int argc, char** argv) {
    const char *name = "", *delta_path = NULL;
    bool verify = false, step = false;
    std::vector<const char*> paths;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--name" && i + 1 < argc)
            name = argv[++i];
        else if (a == "--delta" && i + 1 < argc)
            delta_path = argv[++i];
        else if (a == "--verify")
            verify = true;
        else if (a == "--verify-step")
            step = true;
        else if (a.size() > 1 && a[0] == '-')
            return usage();
        else
            paths.push_back(argv[i]);
    }
    if ((verify && step) || ((verify || step) && (delta_path || *name))) return usage();
    if (paths.size() != (verify ? 1u : 2u)) return usage();
    std::vector<char> first, second;
    if (!read_file(paths[0], first)) {
        fprintf(stderr, "error: cannot read %s\n", paths[0]);
        return 2;
    }
    if (step && !read_file(paths[1], second)) {
        fprintf(stderr, "error: cannot read %s\n", paths[1]);
        return 2;
    }
    gw_status_t st{};
    if (verify) {
        void* image = NULL;  // the record count, from the host-only reader
        size_t image_len = 0;
        if (gwb_zkey_contributions(first.data(), first.size(), &image, &image_len, &st) != 0) return report(2, st);
        uint32_t count;
        memcpy(&count, (const uint8_t*)image + GWB_CONTRIBUTION_HASH_BYTES, 4);
        gwb_groth16_setup_free(image);
        size_t n = count;
        std::vector<uint8_t> hashes(n * GWB_CONTRIBUTION_HASH_BYTES + 1);
        const int rc = gwb_zkey_verify_contributions(first.data(), first.size(), hashes.data(), &n, &st);
        if (rc != 0) return report(rc, st);
        printf("OK! %zu contributions\n", n);
        for (size_t k = 0; k < n; ++k) print_hex(hashes.data() + k * GWB_CONTRIBUTION_HASH_BYTES, GWB_CONTRIBUTION_HASH_BYTES);
        return 0;
    }
    if (step) {
        const int rc = gwb_zkey_verify_step(first.data(), first.size(), second.data(), second.size(), NULL, &st);
        if (rc != 0) return report(rc, st);
        printf("OK! %s is %s after one contribution\n", paths[1], paths[0]);
        return 0;
    }
    uint8_t delta[32];
    if (delta_path && !parse_delta(delta_path, delta)) return 2;
    if (strlen(name) > GWB_CONTRIBUTION_NAME_MAX) {
        fprintf(stderr, "error: the name has more than 255 bytes\n");
        return 2;
    }
    void* out = NULL;
    size_t out_len = 0;
    uint8_t hash[GWB_CONTRIBUTION_HASH_BYTES];
    const int rc = gwb_groth16_contribute(first.data(), first.size(), name, delta_path ? delta : NULL, &out, &out_len, hash, &st);
    memset(delta, 0, sizeof delta);
    if (rc != 0) return report(2, st);
    const bool ok = write_file(paths[1], out, out_len);
    gwb_groth16_setup_free(out);
    if (!ok) {
        fprintf(stderr, "error: cannot write %s\n", paths[1]);
        return 2;
    }
    print_hex(hash, sizeof hash);
    return 0;
}
