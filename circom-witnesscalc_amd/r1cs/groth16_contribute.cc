// groth16-contribute [--name NAME] [--delta FILE] <in.zkey> <out.zkey>: one phase-2 contribution to a Groth16 key, made on the
// GPU (include/graph_witness_groth16_contribute.h).  The secret is drawn and discarded, or read from FILE (one decimal integer
// in [1, r), for reproducible keys).  Prints the contribution hash in hex.
// groth16-contribute --beacon [--name NAME] <in.zkey> <out.zkey> <beaconHash(hex)> <numIterationsExp>: the last contribution of phase 2,
// whose secret nobody chooses: it is derived from the public beaconHash by 2^numIterationsExp chained SHA-256 on the host
// (include/graph_witness_groth16_beacon.h; snarkjs `zkey beacon`, with its argument order).  Prints the record's hash in hex.
// groth16-contribute --verify [--require-beacon] <key.zkey>: checks the key's contribution records and prints their hashes;
// --require-beacon, here and with --verify-key, additionally refuses a key whose last record is not a beacon.
// groth16-contribute --verify-step <prev.zkey> <next.zkey>: checks that next is prev after exactly one contribution.
// groth16-contribute --verify-key [--lagrange auto|file|compute] [--skip-records] [--check-ptau] [--check-lagrange] <circuit.r1cs> <pot.ptau> <key.zkey>:
// checks the key against its circuit and its powers-of-tau file (snarkjs `zkey verify`, with its argument order) and prints the
// hashes of its records.  The file is mapped into memory, not read; --lagrange defaults to compute, which keeps the verdict
// off the file's prepared sections; --skip-records passes over section 10 (a key with snarkjs's records); --check-ptau first
// checks that the points read from the file are powers of one tau; --check-lagrange (with --lagrange auto or file) first checks
// the prepared sections that the remake reads against the monomial ones (gwb_ptau_check_lagrange), and its failure is the verdict.
// The records are this library's own: they are not interchangeable with snarkjs's (see the header).  Exit status 0 on success;
// 1 for a failed verification, with its message; 2 on a usage, file or format error.  Every input is parsed before the device
// is touched.
#include "../../include/graph_witness_groth16_beacon.h"
#include "../../include/graph_witness_groth16_contribute.h"
#include "../../include/graph_witness_groth16_ptau.h"
#include "../../include/graph_witness_groth16_setup.h"
#include "cli_common.hpp"

using cli::print_hex;
using Image = cli::Owned<void, gwb_groth16_setup_free>;  // a key or a list made by the library

static int usage() {
    fprintf(stderr,
            "usage: groth16-contribute [--name NAME] [--delta FILE] <in.zkey> <out.zkey>\n"
            "       groth16-contribute --beacon [--name NAME] <in.zkey> <out.zkey> <beaconHash(hex)> <numIterationsExp>\n"
            "       groth16-contribute --verify <key.zkey>\n"
            "       groth16-contribute --verify --require-beacon <key.zkey>\n"
            "       groth16-contribute --verify-step <prev.zkey> <next.zkey>\n"
            "       groth16-contribute --verify-key [--lagrange auto|file|compute] [--skip-records] [--check-ptau] [--check-lagrange] <circuit.r1cs> <pot.ptau> <key.zkey>\n"
            "       groth16-contribute --verify-key --require-beacon [the options above] <circuit.r1cs> <pot.ptau> <key.zkey>\n");
    return 2;
}

// the number of records of a key and the type of the last one (-1 without records), from the host-only reader; false with st set
static bool record_count(const std::vector<uint8_t>& key, size_t& n, gw_status_t& st, int* last_type = NULL) {
    void* made = NULL;
    size_t image_len = 0;
    if (gwb_zkey_contributions(key.data(), key.size(), &made, &image_len, &st) != 0) return false;
    const Image owner(made);
    const uint8_t* image = (const uint8_t*)made;
    uint32_t count;
    memcpy(&count, image + GWB_CONTRIBUTION_HASH_BYTES, 4);
    if (last_type) {
        *last_type = -1;
        const uint8_t* p = image + GWB_CONTRIBUTION_HASH_BYTES + 4;  // per record: 448 B, u32 type, u32 nameLen, name
        for (uint32_t k = 0; k < count; ++k) {
            uint32_t type, name_len;
            memcpy(&type, p + 448, 4);
            memcpy(&name_len, p + 452, 4);
            *last_type = (int)type;
            p += 456 + name_len;
        }
    }
    n = count;
    return true;
}

static int not_a_beacon() {
    fprintf(stderr, "INVALID: zkey: the last contribution is not a beacon\n");
    return 1;
}

static int report(int rc, gw_status_t& st) { return cli::report(rc, st, "call failed"); }

static int run_verify_key(const char* r1cs_path, const char* ptau_path, const char* key_path, const char* lagrange, bool skip_records, bool check_ptau,
                          bool check_lagrange, bool require_beacon) {
    uint32_t mode = GWB_PTAU_LAGRANGE_COMPUTE;
    if (lagrange) {
        if (strcmp(lagrange, "auto") == 0)
            mode = GWB_PTAU_LAGRANGE_AUTO;
        else if (strcmp(lagrange, "file") == 0)
            mode = GWB_PTAU_LAGRANGE_FILE;
        else if (strcmp(lagrange, "compute") != 0)
            return usage();
    }
    std::vector<uint8_t> circuit, key;
    cli::Mapped ptau;
    const char* unread = !cli::read_file(r1cs_path, circuit) ? r1cs_path : !ptau.open(ptau_path) ? ptau_path : !cli::read_file(key_path, key) ? key_path : NULL;
    if (unread) return cli::cannot_read(unread);
    gw_status_t st{};
    gwb_r1cs_t* loaded = NULL;
    if (gwb_r1cs_load(circuit.data(), circuit.size(), &loaded, &st) != 0) return cli::fail(r1cs_path, st, "load failed");
    const cli::Owned<gwb_r1cs_t, gwb_r1cs_free> r(loaded);
    size_t n = 0;
    int last_type = -1;
    if (!record_count(key, n, st, &last_type)) return report(2, st);
    if (check_lagrange && mode != GWB_PTAU_LAGRANGE_COMPUTE) {  // under auto, only a file that has the sections
        gwb_ptau_info_t pi;
        gwb_r1cs_qap_info_t qi;
        int rc = gwb_ptau_info(ptau.data, ptau.len, &pi, &st) != 0 || gwb_r1cs_qap_info(r.get(), &qi, &st) != 0 ? 2 : 0;
        if (rc == 0 && (mode == GWB_PTAU_LAGRANGE_FILE || pi.prepared)) rc = gwb_ptau_check_lagrange(ptau.data, ptau.len, qi.domain_power, NULL, &st);
        if (rc != 0) return report(rc, st);
    }
    std::vector<uint8_t> hashes(n * GWB_CONTRIBUTION_HASH_BYTES + 1);
    const uint32_t flags = (skip_records ? GWB_VERIFY_KEY_SKIP_RECORDS : 0u) | (check_ptau ? GWB_VERIFY_KEY_CHECK_PTAU : 0u);
    const int rc = gwb_zkey_verify_key(key.data(), key.size(), r.get(), ptau.data, ptau.len, mode, flags, NULL, hashes.data(), &n, &st);
    if (rc != 0) return report(rc, st);
    if (require_beacon && last_type != 1) return not_a_beacon();
    printf("OK! %s is the key of %s and %s, %zu contributions%s\n", key_path, r1cs_path, ptau_path, n, skip_records ? " (not verified)" : "");
    for (size_t k = 0; k < n; ++k) print_hex(hashes.data() + k * GWB_CONTRIBUTION_HASH_BYTES, GWB_CONTRIBUTION_HASH_BYTES);
    return 0;
}

int main(int argc, char** argv) {
    const char *name = "", *delta_path = NULL, *lagrange = NULL;
    bool verify = false, step = false, verify_key = false, skip_records = false, check_ptau = false, check_lagrange = false, beacon = false,
         require_beacon = false;
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
        else if (a == "--verify-key")
            verify_key = true;
        else if (a == "--beacon")
            beacon = true;
        else if (a == "--require-beacon")
            require_beacon = true;
        else if (a == "--skip-records")
            skip_records = true;
        else if (a == "--check-ptau")
            check_ptau = true;
        else if (a == "--check-lagrange")
            check_lagrange = true;
        else if (a == "--lagrange" && i + 1 < argc)
            lagrange = argv[++i];
        else if (a.size() > 1 && a[0] == '-')
            return usage();
        else
            paths.push_back(argv[i]);
    }
    if (verify + step + verify_key + beacon > 1 || ((verify || step || verify_key) && (delta_path || *name)) || (beacon && delta_path)) return usage();
    if (require_beacon && !verify && !verify_key) return usage();
    if (!verify_key && (lagrange || skip_records || check_ptau || check_lagrange)) return usage();
    if (paths.size() != (verify ? 1u : verify_key ? 3u : beacon ? 4u : 2u)) return usage();
    if (verify_key) return run_verify_key(paths[0], paths[1], paths[2], lagrange, skip_records, check_ptau, check_lagrange, require_beacon);
    std::vector<uint8_t> beacon_hash;
    uint32_t beacon_exp = 0;
    if (beacon) {  // the arguments before the key is read
        if (!cli::parse_hex(paths[2], GWB_BEACON_HASH_MAX, beacon_hash)) {
            fprintf(stderr, "error: beaconHash: an even number of hex digits for 1 to 255 bytes expected, without a prefix\n");
            return 2;
        }
        if (!cli::parse_u32(paths[3], 0xffffffffu, beacon_exp)) {
            fprintf(stderr, "error: numIterationsExp: a decimal number expected\n");
            return 2;
        }
    }
    std::vector<uint8_t> first, second;
    if (!cli::read_file(paths[0], first)) return cli::cannot_read(paths[0]);
    if (step && !cli::read_file(paths[1], second)) return cli::cannot_read(paths[1]);
    gw_status_t st{};
    if (verify) {
        size_t n = 0;
        int last_type = -1;
        if (!record_count(first, n, st, &last_type)) return report(2, st);
        std::vector<uint8_t> hashes(n * GWB_CONTRIBUTION_HASH_BYTES + 1);
        const int rc = gwb_zkey_verify_contributions(first.data(), first.size(), hashes.data(), &n, &st);
        if (rc != 0) return report(rc, st);
        if (require_beacon && last_type != 1) return not_a_beacon();
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
    uint8_t delta[1][32];
    cli::Secrets found;
    if (delta_path && !cli::parse_secret_decimals(delta_path, 1, delta, found)) {
        if (!found.readable) return cli::cannot_read(delta_path);
        fprintf(stderr, "error: %s: one decimal integer below 2^256 expected (delta)\n", delta_path);
        return 2;
    }
    if (strlen(name) > GWB_CONTRIBUTION_NAME_MAX) {
        fprintf(stderr, "error: the name has more than 255 bytes\n");
        return 2;
    }
    void* out = NULL;
    size_t out_len = 0;
    uint8_t hash[GWB_CONTRIBUTION_HASH_BYTES];
    const int rc = beacon ? gwb_groth16_beacon(first.data(), first.size(), name, beacon_hash.data(), beacon_hash.size(), beacon_exp, &out, &out_len, hash, &st)
                          : gwb_groth16_contribute(first.data(), first.size(), name, delta_path ? delta[0] : NULL, &out, &out_len, hash, &st);
    explicit_bzero(delta, sizeof delta);
    if (rc != 0) return report(2, st);
    const Image image(out);
    if (!cli::write_file(paths[1], out, out_len)) return cli::cannot_write(paths[1]);
    print_hex(hash, sizeof hash);
    return 0;
}
