// kzg commit <pot.ptau> <poly.bin> <commitment.bin>: C = sum c_i tauG1[i] (include/graph_witness_kzg.h), on the GPU.
// kzg open <pot.ptau> <poly.bin> <z.bin> <y.bin> <proof.bin>: y = p(z) and the witness W of the opening at z.
// kzg verify <pot.ptau> <commitment.bin> <z.bin> <y.bin> <proof.bin>: prints OK! or the status name (SCALAR, POINT, EQUATION).
// Files are raw: a polynomial is its coefficients, 32 bytes little-endian each; z and y are one such scalar; a commitment or a
// proof is one point, 64 bytes canonical little-endian affine x, y (zero bytes: infinity).  The handle covers the polynomial's
// length, or one point for verify.  The `.ptau` is mapped into memory; every input is read, and the sizes checked, before the
// device is touched.  Exit status 0 on success; 1 for a failed check, with its name; 2 on a usage, file or format error.
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/graph_witness_kzg.h"

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

static bool read_file(const char* path, std::vector<uint8_t>& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        fprintf(stderr, "error: cannot read %s\n", path);
        return false;
    }
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

// a file of exactly `bytes` bytes
static bool read_sized(const char* path, size_t bytes, const char* what, std::vector<uint8_t>& out) {
    if (!read_file(path, out)) return false;
    if (out.size() == bytes) return true;
    fprintf(stderr, "error: %s: %zu bytes, %s is %zu\n", path, out.size(), what, bytes);
    return false;
}

static bool write_file(const char* path, const void* data, size_t n) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(data, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

static int usage() {
    fprintf(stderr,
            "usage: kzg commit <pot.ptau> <poly.bin> <commitment.bin>\n"
            "       kzg open <pot.ptau> <poly.bin> <z.bin> <y.bin> <proof.bin>\n"
            "       kzg verify <pot.ptau> <commitment.bin> <z.bin> <y.bin> <proof.bin>\n");
    return 2;
}

static int failed(gw_status_t& st) {
    fprintf(stderr, "error: %s\n", st.error_msg ? st.error_msg : "the call failed");
    free(st.error_msg);
    return 2;
}

int main(int argc, char** argv) {
    if (argc < 2) return usage();
    const std::string cmd = argv[1];
    const bool commit = cmd == "commit", open = cmd == "open", verify = cmd == "verify";
    if (!(commit && argc == 5) && !((open || verify) && argc == 7)) return usage();
    Mapped ptau;
    if (!ptau.open(argv[2])) {
        fprintf(stderr, "error: cannot read %s\n", argv[2]);
        return 2;
    }
    std::vector<uint8_t> poly, c, z, y, w;
    if (verify) {
        if (!read_sized(argv[3], 64, "a commitment", c) || !read_sized(argv[4], 32, "a scalar", z) || !read_sized(argv[5], 32, "a scalar", y) ||
            !read_sized(argv[6], 64, "a proof", w))
            return 2;
    } else {
        if (!read_file(argv[3], poly)) return 2;
        if (poly.empty() || poly.size() % 32 != 0) {
            fprintf(stderr, "error: %s: %zu bytes, a polynomial is a positive number of 32-byte coefficients\n", argv[3], poly.size());
            return 2;
        }
        if (open && !read_sized(argv[4], 32, "a scalar", z)) return 2;
    }
    const size_t n = poly.size() / 32;
    gw_status_t st = {};
    gwb_ptau_info_t pi;
    if (gwb_ptau_info(ptau.data, ptau.len, &pi, &st) != 0) return failed(st);  // (host only: a malformed file ends here)
    gwb_kzg_t* h = NULL;
    if (gwb_kzg_new(ptau.data, ptau.len, verify ? 1 : n, 0, &h, &st) != 0) return failed(st);
    int rc = 0;
    if (commit) {
        c.resize(64);
        if (gwb_kzg_commit_batch(h, poly.data(), 1, n, c.data(), &st) != 0) {
            rc = failed(st);
        } else if (!write_file(argv[4], c.data(), c.size())) {
            fprintf(stderr, "error: cannot write %s\n", argv[4]);
            rc = 2;
        }
    } else if (open) {
        y.resize(32);
        w.resize(64);
        if (gwb_kzg_open_batch(h, poly.data(), z.data(), 1, n, y.data(), w.data(), &st) != 0) {
            rc = failed(st);
        } else if (!write_file(argv[5], y.data(), y.size()) || !write_file(argv[6], w.data(), w.size())) {
            fprintf(stderr, "error: cannot write %s or %s\n", argv[5], argv[6]);
            rc = 2;
        }
    } else {
        uint32_t verdict = 0;
        static const char* names[4] = {"OK!", "SCALAR", "POINT", "EQUATION"};
        if (gwb_kzg_verify_batch(h, c.data(), z.data(), y.data(), w.data(), 1, &verdict, &st) != 0) {
            rc = failed(st);
        } else {
            printf("%s\n", verdict < 4 ? names[verdict] : "?");
            rc = verdict == GWB_KZG_VALID ? 0 : 1;
        }
    }
    gwb_kzg_free(h);
    return rc;
}
