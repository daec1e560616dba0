// What the eight command-line tools of this directory share: the only place in them that opens, maps, reads or writes a file,
// parses a number from text, or takes the message out of a status.  Host only, header only; of the library it knows
// gw_status_t and nothing else, so the owner of a C handle is templated on the handle's free function.  Usage texts, argument
// loops and messages are each tool's own.
#pragma once
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../../include/graph_witness.h"

namespace cli {

// -- files ----------------------------------------------------------------------------------------------------------------------
inline bool read_file(const char* path, std::vector<uint8_t>& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return !f.bad();
}

inline bool write_file(const char* path, const void* data, size_t n) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(data, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

// a file mapped read-only; size 0 maps nothing
struct Mapped {
    void* data = NULL;
    size_t len = 0;
    Mapped() = default;
    Mapped(const Mapped&) = delete;
    Mapped& operator=(const Mapped&) = delete;
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

inline int cannot_read(const char* path) {
    fprintf(stderr, "error: cannot read %s\n", path);
    return 2;
}

inline int cannot_write(const char* path) {
    fprintf(stderr, "error: cannot write %s\n", path);
    return 2;
}

// -- 256-bit decimals -------------------------------------------------------------------------------------------------------------
enum class Decimal { ok, not_decimal, too_large };

// n decimal digits -> 32-byte little-endian integer, written on ok alone; otherwise what is wrong with the leftmost character
// that is wrong: not a digit (or no digit at all), or the value reaches 2^256 there.  The words it works in are wiped.
inline Decimal parse_decimal(const char* s, size_t n, uint8_t* le) {
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    Decimal r = n ? Decimal::ok : Decimal::not_decimal;
    for (size_t k = 0; k < n && r == Decimal::ok; ++k) {
        if (s[k] < '0' || s[k] > '9') {
            r = Decimal::not_decimal;
            break;
        }
        uint64_t carry = (uint64_t)(s[k] - '0');
        for (int i = 0; i < 8; ++i) {
            const uint64_t cur = (uint64_t)w[i] * 10 + carry;
            w[i] = (uint32_t)cur;
            carry = cur >> 32;
        }
        if (carry) r = Decimal::too_large;
    }
    if (r == Decimal::ok) memcpy(le, w, 32);
    explicit_bzero(w, sizeof w);
    return r;
}

// 32-byte little-endian integer -> decimal string
inline std::string decimal(const uint8_t* le) {
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

// what parse_secret_decimals found: the tools word their own messages from it
struct Secrets {
    static constexpr size_t none = (size_t)-1;
    bool readable = false;
    size_t tokens = 0;  // in the whole file
    size_t bad = none;  // the first of the n_wanted first tokens that is not a decimal integer below 2^256
};

// A file of secrets: n_wanted decimal integers below 2^256 separated by spaces, tabs, \n or \r -> le[0 .. n_wanted), written
// only when the file holds exactly that (the return value); the caller wipes le after use.  The file's text and the values
// staged here are wiped on every path, and no digit is copied anywhere else.
inline bool parse_secret_decimals(const char* path, size_t n_wanted, uint8_t (*le)[32], Secrets& found) {
    found = Secrets();
    std::vector<uint8_t> text, staged(32 * n_wanted);
    found.readable = read_file(path, text);
    for (size_t i = 0; found.readable && i < text.size();) {
        auto space = [&](size_t k) { return text[k] == ' ' || text[k] == '\n' || text[k] == '\r' || text[k] == '\t'; };
        if (space(i)) {
            ++i;
            continue;
        }
        size_t end = i;
        while (end < text.size() && !space(end)) ++end;
        if (found.tokens < n_wanted && found.bad == Secrets::none &&
            parse_decimal((const char*)text.data() + i, end - i, staged.data() + 32 * found.tokens) != Decimal::ok)
            found.bad = found.tokens;
        ++found.tokens;
        i = end;
    }
    const bool ok = found.readable && found.tokens == n_wanted && found.bad == Secrets::none;
    if (ok) memcpy(le, staged.data(), staged.size());
    if (!text.empty()) explicit_bzero(text.data(), text.size());
    if (!staged.empty()) explicit_bzero(staged.data(), staged.size());
    return ok;
}

// -- arguments --------------------------------------------------------------------------------------------------------------------
// an even number of hex digits, either case, no prefix, 1 to max_bytes bytes
inline bool parse_hex(const char* text, size_t max_bytes, std::vector<uint8_t>& out) {
    const size_t n = strlen(text);
    if (n == 0 || n % 2 != 0 || n / 2 > max_bytes) return false;
    out.assign(n / 2, 0);
    for (size_t i = 0; i < n; ++i) {
        const char c = text[i];
        const int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
        if (v < 0) return false;
        out[i / 2] = (uint8_t)(out[i / 2] << 4 | v);
    }
    return true;
}

inline void print_hex(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
    printf("\n");
}

// a decimal number up to max, as strtoul reads it, but not an empty text, one that goes on after the number, or a leading '-'
inline bool parse_u32(const char* text, uint32_t max, uint32_t& out) {
    char* end = NULL;
    const unsigned long v = strtoul(text, &end, 10);
    if (!*text || *end || text[0] == '-' || v > max) return false;
    out = (uint32_t)v;
    return true;
}

// -- statuses ---------------------------------------------------------------------------------------------------------------------
// the status's message, or the fallback; the status is left empty
inline std::string take_message(gw_status_t& st, const char* fallback) {
    const std::string m = st.error_msg ? st.error_msg : fallback;
    free(st.error_msg);
    st.error_msg = NULL;
    return m;
}

// "error: PATH: MSG", exit status 2
inline int fail(const char* path, gw_status_t& st, const char* fallback) {
    fprintf(stderr, "error: %s: %s\n", path, take_message(st, fallback).c_str());
    return 2;
}

// "INVALID: MSG" and exit status 1 for a call that returned 1 (a failed verification), "error: MSG" and 2 for any other
inline int report(int rc, gw_status_t& st, const char* fallback) {
    fprintf(stderr, "%s: %s\n", rc == 1 ? "INVALID" : "error", take_message(st, fallback).c_str());
    return rc == 1 ? 1 : 2;
}

// -- owners -----------------------------------------------------------------------------------------------------------------------
// a C handle or a malloc'ed image with the function that frees it: Owned<gwb_r1cs_t, gwb_r1cs_free>
template <auto Free>
struct Freeing {
    template <class T>
    void operator()(T* p) const {
        Free(p);
    }
};
template <class T, auto Free>
using Owned = std::unique_ptr<T, Freeing<Free>>;

}  // namespace cli
