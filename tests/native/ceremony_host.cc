// Host-only sanitizer harness for section 7 of a `.ptau` (r1cs/ceremony.cc's reader, through gwb_ptau_contributions): built with
// -fsanitize=address,undefined by tests/test_ptau_ceremony_host.py together with ceremony.cc, ptau.cc and contributions.cc, no
// HIP and no device.  argv[1] is a `.ptau` whose last section is section 7.  The program reads it, then feeds the reader the file
// itself, the file with every third prefix of section 7's body in place of the body, and argv[2] files with one byte of the body
// replaced (position and value from xorshift64 with the seed 88172645463325252, position first); every image lives in a heap
// block of exactly its size, so a read past its end is seen.  It prints one line per case: the return code and the message.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../circom-witnesscalc_amd/r1cs/r1cs_internal.hpp"
#include "../../include/graph_witness_groth16_ceremony.h"

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

static void run_case(const std::vector<uint8_t>& head, const uint8_t* body, uint64_t size) {
    const size_t len = head.size() + 8 + size;
    uint8_t* image = (uint8_t*)malloc(len);  // exactly the file
    memcpy(image, head.data(), head.size());
    memcpy(image + head.size(), &size, 8);
    if (size) memcpy(image + head.size() + 8, body, size);
    gw_status_t st{};
    void* out = nullptr;
    size_t out_len = 0;
    const int rc = gwb_ptau_contributions(image, len, &out, &out_len, &st);
    printf("%d %s\n", rc, rc == 0 ? std::to_string(out_len).c_str() : st.error_msg ? st.error_msg : "");
    free(st.error_msg);
    gwb_groth16_setup_free(out);
    free(image);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<uint8_t> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    uint32_t n_sections;
    memcpy(&n_sections, file.data() + 8, 4);
    size_t off = 12;
    for (uint32_t i = 0; i + 1 < n_sections; ++i) {
        uint64_t size;
        memcpy(&size, file.data() + off + 4, 8);
        off += 12 + size;
    }
    uint32_t id;
    memcpy(&id, file.data() + off, 4);
    if (id != 7) return 2;
    const std::vector<uint8_t> head(file.begin(), file.begin() + off + 4), body(file.begin() + off + 12, file.end());
    run_case(head, body.data(), body.size());
    for (size_t cut = 0; cut < body.size(); cut += 3) run_case(head, body.data(), cut);
    uint64_t x = 88172645463325252ull;
    auto next = [&x]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    const long flips = strtol(argv[2], nullptr, 10);
    for (long i = 0; i < flips; ++i) {
        std::vector<uint8_t> b = body;
        const size_t at = next() % b.size();
        b[at] = (uint8_t)next();
        run_case(head, b.data(), b.size());
    }
    return 0;
}
