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
#include "../../include/graph_witness_groth16_beacon.h"
#include "../../include/graph_witness_groth16_ceremony.h"
#include "../../include/graph_witness_groth16_setup.h"
#include "cli_common.hpp"

using cli::cannot_read;
using cli::Mapped;
using cli::print_hex;
using Image = cli::Owned<void, gwb_groth16_setup_free>;  // a file or a list made by the library

// the type of the file's last record, or -1 without records; false with st set
static bool last_record_type(const void* data, size_t len, uint32_t n_records, int& type, gw_status_t& st) {
    void* made = NULL;
    size_t image_len = 0;
    if (gwb_ptau_contributions(data, len, &made, &image_len, &st) != 0) return false;
    const Image image(made);
    const uint8_t* p = (const uint8_t*)made + 4;  // per record: 1216 B of points, 64 B nextChallenge, u32 type, u32 nameLen, name
    type = -1;
    for (uint32_t k = 0; k < n_records; ++k) {
        uint32_t t, name_len;
        memcpy(&t, p + 1216 + 64, 4);
        memcpy(&name_len, p + 1216 + 64 + 4, 4);
        type = (int)t;
        p += 1216 + 64 + 8 + name_len;
    }
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

static int report(int rc, gw_status_t& st) { return cli::report(rc, st, "call failed"); }

static int write_out(const char* path, void* out, size_t out_len) {
    const Image image(out);
    return cli::write_file(path, out, out_len) ? 0 : cli::cannot_write(path);
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
        uint32_t power = 0;
        if (!cli::parse_u32(paths[0], 0xffffffffu, power)) return usage();
        if (gwb_ptau_new(power, &out, &out_len, &st) != 0) return report(2, st);
        return write_out(paths[1], out, out_len);
    }
    if (cmd == "contribute") {
        if (paths.size() != 2) return usage();
        Mapped in;
        if (!in.open(paths[0])) return cannot_read(paths[0]);
        uint8_t secrets[3][32];
        cli::Secrets found;
        if (secrets_path && !cli::parse_secret_decimals(secrets_path, 3, secrets, found)) {
            if (!found.readable) return cannot_read(secrets_path);
            fprintf(stderr, "error: %s: three decimal integers below 2^256 expected (tau, alpha, beta)\n", secrets_path);
            return 2;
        }
        if (strlen(name) > GWB_CONTRIBUTION_NAME_MAX) {
            fprintf(stderr, "error: the name has more than 255 bytes\n");
            return 2;
        }
        uint8_t hash[GWB_CONTRIBUTION_HASH_BYTES];
        const int rc = gwb_ptau_contribute(in.data, in.len, name, secrets_path ? secrets[0] : NULL, &out, &out_len, hash, &st);
        explicit_bzero(secrets, sizeof secrets);
        if (rc != 0) return report(2, st);
        if (write_out(paths[1], out, out_len) != 0) return 2;
        print_hex(hash, sizeof hash);
        return 0;
    }
    if (cmd == "beacon") {
        if (paths.size() != 4) return usage();
        std::vector<uint8_t> beacon_hash;
        if (!cli::parse_hex(paths[2], GWB_BEACON_HASH_MAX, beacon_hash)) {
            fprintf(stderr, "error: beaconHash: an even number of hex digits for 1 to 255 bytes expected, without a prefix\n");
            return 2;
        }
        uint32_t exp = 0;
        if (!cli::parse_u32(paths[3], 0xffffffffu, exp)) {
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
        void* made = NULL;
        size_t image_len = 0;
        if (gwb_ptau_contributions(next.data, next.len, &made, &image_len, &st) != 0) return report(2, st);
        const Image image(made);
        // the new record is the last: its nextChallenge precedes u32 type, u32 nameLen and the name at the image's end
        const uint8_t* p = (const uint8_t*)made + 4;
        const uint8_t* hash = NULL;
        for (uint32_t k = 0; k < info.n_contributions; ++k) {
            hash = p + 1216;
            uint32_t name_len;
            memcpy(&name_len, p + 1216 + 64 + 4, 4);
            p += 1216 + 64 + 8 + name_len;
        }
        if (hash) print_hex(hash, GWB_CONTRIBUTION_HASH_BYTES);
        return 0;
    }
    return usage();
}
