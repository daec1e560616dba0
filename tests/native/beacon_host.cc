// Host-only sanitizer harness for the random beacon (r1cs/beacon.hpp): built with -fsanitize=address,undefined by
// tests/test_beacon_host.py together with ceremony.cc, ptau.cc and contributions.cc, no HIP and no device.
//   beacon_host <beaconHash hex> <numIterationsExp> <name> <flips>
// It checks SHA-256 against the FIPS 180-4 vectors and the chain's one-block links against the general function, then prints
//   chain <D hex>      scalars1 <6 x 64 hex digits>      scalars2 <2 x 64 hex digits>      (little-endian bytes)
// and one line per parameter image: the beacon's own parameters from write_params, each of their prefixes, and <flips> images with
// one byte replaced (position and value from xorshift64 with the seed 88172645463325252, position first).  Every image lives in
// a heap block of exactly its size, so a read past its end is seen.  A line is
//   <read_params ok> <n_exp> <n_hash> <exp> <hash_len> <form rc under the limit 28>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../circom-witnesscalc_amd/r1cs/beacon.hpp"
#include "../../circom-witnesscalc_amd/r1cs/r1cs_internal.hpp"

// what the library's other objects define for ceremony.cc, ptau.cc and contributions.cc
namespace cwc_r1cs {
void set_status(gw_status_t* st, const std::string& msg) {
    if (!st) return;
    st->error_msg = (char*)malloc(msg.size() + 1);
    memcpy(st->error_msg, msg.c_str(), msg.size() + 1);
}
void set_ok(gw_status_t* st) {
    if (st) st->error_msg = nullptr;
}
int fail(gw_status_t* st, const std::string& msg) {
    set_status(st, msg);
    return 1;
}
}  // namespace cwc_r1cs
extern "C" void gwb_groth16_setup_free(void* p) { free(p); }

static std::string hex(const uint8_t* p, size_t n) {
    static const char* digits = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) {
        s += digits[p[i] >> 4];
        s += digits[p[i] & 15];
    }
    return s;
}

static bool sha_is(const std::string& msg, const char* want) {
    uint8_t d[32];
    uint8_t* exact = (uint8_t*)malloc(msg.size() ? msg.size() : 1);  // exactly the message
    memcpy(exact, msg.data(), msg.size());
    cwc_beacon::sha256(exact, msg.size(), d);
    free(exact);
    return hex(d, 32) == want;
}

static void params_case(const uint8_t* body, size_t size) {
    uint8_t* exact = (uint8_t*)malloc(size ? size : 1);
    if (size) memcpy(exact, body, size);
    cwc_beacon::Items it;
    const bool ok = cwc_beacon::read_params(exact, size, it);
    const cwc_beacon::Form f = cwc_beacon::form_of(std::vector<uint8_t>(exact, exact + size), 28);
    printf("%d %u %u %u %zu %d\n", ok ? 1 : 0, it.n_exp, it.n_hash, it.exp, it.hash_len, f.rc);
    free(exact);
}

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    if (!sha_is("", "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855") ||
        !sha_is("abc", "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad") ||
        !sha_is("abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1") ||
        !sha_is(std::string(1000000, 'a'), "cdc76e5c9914fb9281a1c7e284d73e67f1809a48a497200e046d39ccc7112cd0")) {
        printf("a SHA-256 vector fails\n");
        return 1;
    }
    std::vector<uint8_t> hash;
    for (size_t i = 0; argv[1][i] && argv[1][i + 1]; i += 2) hash.push_back((uint8_t)strtoul(std::string(argv[1] + i, 2).c_str(), nullptr, 16));
    const uint32_t exp = (uint32_t)strtoul(argv[2], nullptr, 10);
    const std::string name = argv[3];
    if (hash.empty() || hash.size() > 255 || exp < 10 || exp > 20 || name.size() > 255) return 2;

    // the chain's links of one block against the general function
    uint8_t D[32], naive[32];
    cwc_beacon::chain(hash.data(), hash.size(), exp, D);
    cwc_beacon::sha256(hash.data(), hash.size(), naive);
    for (uint64_t i = 1; i < (1ull << exp); ++i) cwc_beacon::sha256(naive, 32, naive);
    if (memcmp(D, naive, 32) != 0) {
        printf("the chain is not the repeated hash\n");
        return 1;
    }
    printf("chain %s\n", hex(D, 32).c_str());
    for (uint32_t phase = 1; phase <= 2; ++phase) {
        cwc::Fr x[cwc_beacon::PHASE1_SCALARS];
        cwc_beacon::scalars(phase, hash.data(), hash.size(), exp, x);
        printf("scalars%u", phase);
        for (uint32_t j = 0; j < cwc_beacon::scalar_count(phase); ++j) printf(" %s", hex((const uint8_t*)x[j].v, 32).c_str());
        printf("\n");
    }

    const std::vector<uint8_t> body = cwc_beacon::write_params(name, exp, hash.data(), hash.size());
    printf("params %s\n", hex(body.data(), body.size()).c_str());
    params_case(body.data(), body.size());
    for (size_t cut = 0; cut < body.size(); ++cut) params_case(body.data(), cut);
    uint64_t x = 88172645463325252ull;
    auto next = [&x]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    const long flips = strtol(argv[4], nullptr, 10);
    for (long i = 0; i < flips; ++i) {
        std::vector<uint8_t> b = body;
        const size_t at = next() % b.size();
        b[at] = (uint8_t)next();
        params_case(b.data(), b.size());
    }
    return 0;
}
