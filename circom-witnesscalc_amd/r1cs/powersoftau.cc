// powersoftau new POWER <out.ptau>: a new ceremony file, tau = alpha = beta = 1 (include/graph_witness_groth16_ceremony.h; host only).
// powersoftau contribute [--name NAME] [--secrets FILE] <in.ptau> <out.ptau>: one contribution, made on the GPU.  The secrets
// are drawn and discarded, or read from FILE (three decimal integers in [1, r): tau', alpha', beta', for reproducible files).
// Prints the contribution's hash (the record's nextChallenge) in hex.
// powersoftau beacon [--name NAME] <in.ptau> <out.ptau> <beaconHash(hex)> <numIterationsExp>: the ceremony's last contribution, whose
// secrets nobody chooses: they are derived from the public beaconHash by 2^numIterationsExp chained SHA-256 on the host
// (include/graph_witness_groth16_beacon.h; snarkjs's argument order).  Prints the record's hash in hex.
// powersoftau verify [--skip-records] [--require-beacon] <file.ptau>: checks the file's records and that the whole file holds powers
// of one tau, and prints the hashes; --skip-records passes over section 7 (a file with snarkjs's records); --require-beacon
// additionally refuses a file whose last record is not a beacon.
// powersoftau verify-step <prev.ptau> <next.ptau>: checks that next is prev after exactly one contribution.
// The records are this library's own: they are not interchangeable with snarkjs's (see the header).  Inputs are mapped into
// memory and parsed before the device is touched.  Exit status 0 on success; 1 for a failed verification, with its message; 2 on
// a usage, file or format error.
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/graph_witness_groth16_beacon.h"
#include "../../include/graph_witness_groth16_ceremony.h"
#include "../../include/graph_witness_groth16_setup.h"

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

static bool write_file(const char* path, const void* data, size_t n) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(data, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

// a file with three decimal integers below 2^256 -> 96 little-endian bytes; the file's text is zeroed
static bool parse_secrets(const char* path, uint8_t* le) {
    std::vector<char> text;
    {
        std::ifstream f(path, std::ios::binary);
        if (!f) {
            fprintf(stderr, "error: cannot read %s\n", path);
            return false;
        }
        text.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    }
    uint32_t w[3][8] = {};
    size_t tokens = 0;
    bool ok = true, in_token = false;
    for (char c : text) {
        if (c == ' ' || c == '\n' || c == '\r' || c == '\t') {
            in_token = false;
            continue;
        }
        if (!in_token) ++tokens;
        in_token = true;
        if (c < '0' || c > '9' || tokens > 3) {
            ok = false;
            break;
        }
        uint32_t* x = w[tokens - 1];
        uint64_t carry = (uint64_t)(c - '0');
        for (int i = 0; i < 8; ++i) {
            const uint64_t cur = (uint64_t)x[i] * 10 + carry;
            x[i] = (uint32_t)cur;
            carry = cur >> 32;
        }
        if (carry) ok = false;
    }
    std::fill(text.begin(), text.end(), 0);
    if (ok && tokens == 3) memcpy(le, w, 96);
    memset(w, 0, sizeof w);
    if (!ok || tokens != 3) {
        fprintf(stderr, "error: %s: three decimal integers below 2^256 expected (tau, alpha, beta)\n", path);
        return false;
    }
    return true;
}

static void print_hex(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
    printf("\n");
}

// an even number of hex digits, either case, no prefix, 1 to 255 bytes
static bool parse_hex(const char* text, std::vector<uint8_t>& out) {
    const size_t n = strlen(text);
    if (n == 0 || n % 2 != 0 || n / 2 > GWB_BEACON_HASH_MAX) return false;
    out.assign(n / 2, 0);
    for (size_t i = 0; i < n; ++i) {
        const char c = text[i];
        const int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
        if (v < 0) return false;
        out[i / 2] = (uint8_t)(out[i / 2] << 4 | v);
    }
    return true;
}

// the type of the file's last record, or -1 without records; false with st set
static bool last_record_type(const void* data, size_t len, uint32_t n_records, int& type, gw_status_t& st) {
    void* image = NULL;
    size_t image_len = 0;
    if (gwb_ptau_contributions(data, len, &image, &image_len, &st) != 0) return false;
    const uint8_t* p = (const uint8_t*)image + 4;  // per record: 1216 B of points, 64 B nextChallenge, u32 type, u32 nameLen, name
    type = -1;
    for (uint32_t k = 0; k < n_records; ++k) {
        uint32_t t, name_len;
        memcpy(&t, p + 1216 + 64, 4);
        memcpy(&name_len, p + 1216 + 64 + 4, 4);
        type = (int)t;
        p += 1216 + 64 + 8 + name_len;
    }
    gwb_groth16_setup_free(image);
    return true;
}

static int usage() {
    fprintf(stderr,
            "usage: powersoftau new POWER <out.ptau>\n"
            "       powersoftau contribute [--name NAME] [--secrets FILE] <in.ptau> <out.ptau>\n"
            "       powersoftau beacon [--name NAME] <in.ptau> <out.ptau> <beaconHash(hex)> <numIterationsExp>\n"
            "       powersoftau verify [--skip-records] <file.ptau>\n"
            "       powersoftau verify [--skip-records] --require-beacon <file.ptau>\n"
            "       powersoftau verify-step <prev.ptau> <next.ptau>\n");
    return 2;
}

static int report(int rc, gw_status_t& st) {
    fprintf(stderr, "%s: %s\n", rc == 1 ? "INVALID" : "error", st.error_msg ? st.error_msg : "call failed");
    free(st.error_msg);
    return rc == 1 ? 1 : 2;
}

static int cannot_read(const char* path) {
    fprintf(stderr, "error: cannot read %s\n", path);
    return 2;
}

static int write_out(const char* path, void* out, size_t out_len) {
    const bool ok = write_file(path, out, out_len);
    gwb_groth16_setup_free(out);
    if (!ok) fprintf(stderr, "error: cannot write %s\n", path);
    return ok ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc < 2) return usage();
    const std::string cmd = argv[1];
    const char *name = "", *secrets_path = NULL;
    bool skip_records = false, require_beacon = false;
    std::vector<const char*> paths;
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--name" && i + 1 < argc && (cmd == "contribute" || cmd == "beacon"))
            name = argv[++i];
        else if (a == "--secrets" && i + 1 < argc && cmd == "contribute")
            secrets_path = argv[++i];
        else if (a == "--skip-records" && cmd == "verify")
            skip_records = true;
        else if (a == "--require-beacon" && cmd == "verify")
            require_beacon = true;
        else if (a.size() > 1 && a[0] == '-')
            return usage();
        else
            paths.push_back(argv[i]);
    }
    gw_status_t st{};
    void* out = NULL;
    size_t out_len = 0;
    if (cmd == "new") {
        if (paths.size() != 2) return usage();
        char* end = NULL;
        const unsigned long power = strtoul(paths[0], &end, 10);
        if (!*paths[0] || *end || power > 0xfffffffful) return usage();
        if (gwb_ptau_new((uint32_t)power, &out, &out_len, &st) != 0) return report(2, st);
        return write_out(paths[1], out, out_len);
    }
    if (cmd == "contribute") {
        if (paths.size() != 2) return usage();
        Mapped in;
        if (!in.open(paths[0])) return cannot_read(paths[0]);
        uint8_t secrets[96];
        if (secrets_path && !parse_secrets(secrets_path, secrets)) return 2;
        if (strlen(name) > GWB_CONTRIBUTION_NAME_MAX) {
            fprintf(stderr, "error: the name has more than 255 bytes\n");
            return 2;
        }
        uint8_t hash[GWB_CONTRIBUTION_HASH_BYTES];
        const int rc = gwb_ptau_contribute(in.data, in.len, name, secrets_path ? secrets : NULL, &out, &out_len, hash, &st);
        memset(secrets, 0, sizeof secrets);
        if (rc != 0) return report(2, st);
        if (write_out(paths[1], out, out_len) != 0) return 2;
        print_hex(hash, sizeof hash);
        return 0;
    }
    if (cmd == "beacon") {
        if (paths.size() != 4) return usage();
        std::vector<uint8_t> beacon_hash;
        if (!parse_hex(paths[2], beacon_hash)) {
            fprintf(stderr, "error: beaconHash: an even number of hex digits for 1 to 255 bytes expected, without a prefix\n");
            return 2;
        }
        char* end = NULL;
        const unsigned long exp = strtoul(paths[3], &end, 10);
        if (!*paths[3] || *end || paths[3][0] == '-' || exp > 0xfffffffful) {
            fprintf(stderr, "error: numIterationsExp: a decimal number expected\n");
            return 2;
        }
        if (strlen(name) > GWB_CONTRIBUTION_NAME_MAX) {
            fprintf(stderr, "error: the name has more than 255 bytes\n");
            return 2;
        }
        Mapped in;
        if (!in.open(paths[0])) return cannot_read(paths[0]);
        uint8_t hash[GWB_CONTRIBUTION_HASH_BYTES];
        if (gwb_ptau_beacon(in.data, in.len, name, beacon_hash.data(), beacon_hash.size(), (uint32_t)exp, &out, &out_len, hash, &st) != 0) return report(2, st);
        if (write_out(paths[1], out, out_len) != 0) return 2;
        print_hex(hash, sizeof hash);
        return 0;
    }
    if (cmd == "verify") {
        if (paths.size() != 1) return usage();
        Mapped in;
        if (!in.open(paths[0])) return cannot_read(paths[0]);
        gwb_ptau_info_t info;
        if (gwb_ptau_info(in.data, in.len, &info, &st) != 0) return report(2, st);
        size_t n = info.n_contributions;
        std::vector<uint8_t> hashes(n * GWB_CONTRIBUTION_HASH_BYTES + 1);
        const int rc = gwb_ptau_verify(in.data, in.len, skip_records ? GWB_PTAU_VERIFY_SKIP_RECORDS : 0u, NULL, hashes.data(), &n, &st);
        if (rc != 0) return report(rc, st);
        if (require_beacon) {
            int type = -1;
            if (!last_record_type(in.data, in.len, info.n_contributions, type, st)) return report(2, st);
            if (type != 1) {
                fprintf(stderr, "INVALID: ptau: the last contribution is not a beacon\n");
                return 1;
            }
        }
        printf("OK! power %u, %zu contributions%s\n", info.power, n, skip_records ? " (not verified)" : "");
        for (size_t k = 0; k < n && k < info.n_contributions; ++k) print_hex(hashes.data() + k * GWB_CONTRIBUTION_HASH_BYTES, GWB_CONTRIBUTION_HASH_BYTES);
        return 0;
    }
    if (cmd == "verify-step") {
        if (paths.size() != 2) return usage();
        Mapped prev, next;
        if (!prev.open(paths[0])) return cannot_read(paths[0]);
        if (!next.open(paths[1])) return cannot_read(paths[1]);
        const int rc = gwb_ptau_verify_step(prev.data, prev.len, next.data, next.len, NULL, &st);
        if (rc != 0) return report(rc, st);
        gwb_ptau_info_t info;
        if (gwb_ptau_info(next.data, next.len, &info, &st) != 0) return report(2, st);
        printf("OK! %s is %s after one contribution\n", paths[1], paths[0]);
        void* image = NULL;
        size_t image_len = 0;
        if (gwb_ptau_contributions(next.data, next.len, &image, &image_len, &st) != 0) return report(2, st);
        // the new record is the last: its nextChallenge precedes u32 type, u32 nameLen and the name at the image's end
        const uint8_t* p = (const uint8_t*)image + 4;
        const uint8_t* hash = NULL;
        for (uint32_t k = 0; k < info.n_contributions; ++k) {
            hash = p + 1216;
            uint32_t name_len;
            memcpy(&name_len, p + 1216 + 64 + 4, 4);
            p += 1216 + 64 + 8 + name_len;
        }
        if (hash) print_hex(hash, GWB_CONTRIBUTION_HASH_BYTES);
        gwb_groth16_setup_free(image);
        return 0;
    }
    return usage();
}
