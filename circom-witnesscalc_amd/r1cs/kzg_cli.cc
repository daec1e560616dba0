// kzg commit <pot.ptau> <poly.bin> <commitment.bin>: C = sum c_i tauG1[i] (include/graph_witness_kzg.h), on the GPU.
// kzg open <pot.ptau> <poly.bin> <z.bin> <y.bin> <proof.bin>: y = p(z) and the witness W of the opening at z.
// kzg verify <pot.ptau> <commitment.bin> <z.bin> <y.bin> <proof.bin>: prints OK! or the status name (SCALAR, POINT, EQUATION).
// kzg open-fold <pot.ptau> <z.bin> <gamma.bin> <ys.bin> <proof.bin> <poly0.bin> [<poly1.bin> ...]: the K polynomials' values at z,
// K x 32 bytes, and the one witness of their fold with the powers of gamma.  The files have one size.
// kzg verify-fold <pot.ptau> <commitments.bin> <z.bin> <gamma.bin> <ys.bin> <proof.bin>: K x 64 bytes of commitments and K x 32 bytes of
// values; prints as verify does.  gamma is the caller's challenge: it has to have been fixed after the commitments, z and the values.
// Files are raw: a polynomial is its coefficients, 32 bytes little-endian each; z and y are one such scalar; a commitment or a
// proof is one point, 64 bytes canonical little-endian affine x, y (zero bytes: infinity).  The handle covers the polynomial's
// length, or one point for verify.  The `.ptau` is mapped into memory; every input is read, and the sizes checked, before the
// device is touched.  Exit status 0 on success; 1 for a failed check, with its name; 2 on a usage, file or format error.
#include "../../include/graph_witness_kzg.h"
#include "cli_common.hpp"

using cli::write_file;

// the file's bytes; false with the message printed
static bool read_file(const char* path, std::vector<uint8_t>& out) {
    if (cli::read_file(path, out)) return true;
    cli::cannot_read(path);
    return false;
}

// a file of exactly `bytes` bytes
static bool read_sized(const char* path, size_t bytes, const char* what, std::vector<uint8_t>& out) {
    if (!read_file(path, out)) return false;
    if (out.size() == bytes) return true;
    fprintf(stderr, "error: %s: %zu bytes, %s is %zu\n", path, out.size(), what, bytes);
    return false;
}

// a polynomial: a positive number of 32-byte coefficients
static bool read_poly(const char* path, std::vector<uint8_t>& out) {
    if (!read_file(path, out)) return false;
    if (!out.empty() && out.size() % 32 == 0) return true;
    fprintf(stderr, "error: %s: %zu bytes, a polynomial is a positive number of 32-byte coefficients\n", path, out.size());
    return false;
}

static int usage() {
    fprintf(stderr,
            "usage: kzg commit <pot.ptau> <poly.bin> <commitment.bin>\n"
            "       kzg open <pot.ptau> <poly.bin> <z.bin> <y.bin> <proof.bin>\n"
            "       kzg verify <pot.ptau> <commitment.bin> <z.bin> <y.bin> <proof.bin>\n"
            "       kzg open-fold <pot.ptau> <z.bin> <gamma.bin> <ys.bin> <proof.bin> <poly0.bin> [<poly1.bin> ...]\n"
            "       kzg verify-fold <pot.ptau> <commitments.bin> <z.bin> <gamma.bin> <ys.bin> <proof.bin>\n");
    return 2;
}

static int failed(gw_status_t& st) { return cli::report(2, st, "the call failed"); }

static int verdict_of(uint32_t verdict) {
    static const char* names[4] = {"OK!", "SCALAR", "POINT", "EQUATION"};
    printf("%s\n", verdict < 4 ? names[verdict] : "?");
    return verdict == GWB_KZG_VALID ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc < 2) return usage();
    const std::string cmd = argv[1];
    const bool commit = cmd == "commit", open = cmd == "open", verify = cmd == "verify", open_fold = cmd == "open-fold", verify_fold = cmd == "verify-fold";
    if (!(commit && argc == 5) && !((open || verify) && argc == 7) && !(open_fold && argc >= 8) && !(verify_fold && argc == 8)) return usage();
    cli::Mapped ptau;
    if (!ptau.open(argv[2])) return cli::cannot_read(argv[2]);
    std::vector<uint8_t> poly, c, z, gamma, y, w;  // (poly: the K polynomials of open-fold one after another)
    size_t n = 0, k = 1;
    if (verify) {
        if (!read_sized(argv[3], 64, "a commitment", c) || !read_sized(argv[4], 32, "a scalar", z) || !read_sized(argv[5], 32, "a scalar", y) ||
            !read_sized(argv[6], 64, "a proof", w))
            return 2;
    } else if (verify_fold) {
        if (!read_file(argv[3], c)) return 2;
        if (c.empty() || c.size() % 64 != 0) {
            fprintf(stderr, "error: %s: %zu bytes, the commitments are a positive number of 64-byte points\n", argv[3], c.size());
            return 2;
        }
        k = c.size() / 64;
        if (!read_sized(argv[4], 32, "a scalar", z) || !read_sized(argv[5], 32, "a scalar", gamma) ||
            !read_sized(argv[6], k * 32, "a value per commitment", y) || !read_sized(argv[7], 64, "a proof", w))
            return 2;
    } else if (open_fold) {
        if (!read_sized(argv[3], 32, "a scalar", z) || !read_sized(argv[4], 32, "a scalar", gamma)) return 2;
        k = (size_t)argc - 7;
        for (size_t i = 0; i < k; ++i) {
            std::vector<uint8_t> one;
            if (!read_poly(argv[7 + i], one)) return 2;
            if (i && one.size() != poly.size() / i) {
                fprintf(stderr, "error: %s: %zu bytes, %s has %zu: the polynomials of a group have one length (pad with zeros)\n", argv[7 + i], one.size(), argv[7],
                        poly.size() / i);
                return 2;
            }
            poly.insert(poly.end(), one.begin(), one.end());
        }
        n = poly.size() / k / 32;
    } else {
        if (!read_poly(argv[3], poly)) return 2;
        if (open && !read_sized(argv[4], 32, "a scalar", z)) return 2;
        n = poly.size() / 32;
    }
    gw_status_t st = {};
    gwb_ptau_info_t pi;
    if (gwb_ptau_info(ptau.data, ptau.len, &pi, &st) != 0) return failed(st);  // (host only: a malformed file ends here)
    gwb_kzg_t* h = NULL;
    if (gwb_kzg_new(ptau.data, ptau.len, verify || verify_fold ? 1 : n, 0, &h, &st) != 0) return failed(st);
    int rc = 0;
    if (commit) {
        c.resize(64);
        if (gwb_kzg_commit_batch(h, poly.data(), 1, n, c.data(), &st) != 0) {
            rc = failed(st);
        } else if (!write_file(argv[4], c.data(), c.size())) {
            rc = cli::cannot_write(argv[4]);
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
    } else if (open_fold) {
        y.resize(k * 32);
        w.resize(64);
        if (gwb_kzg_open_fold_batch(h, poly.data(), z.data(), gamma.data(), 1, k, n, y.data(), w.data(), &st) != 0) {
            rc = failed(st);
        } else if (!write_file(argv[5], y.data(), y.size()) || !write_file(argv[6], w.data(), w.size())) {
            fprintf(stderr, "error: cannot write %s or %s\n", argv[5], argv[6]);
            rc = 2;
        }
    } else {
        uint32_t verdict = 0;
        const int e = verify ? gwb_kzg_verify_batch(h, c.data(), z.data(), y.data(), w.data(), 1, &verdict, &st)
                             : gwb_kzg_verify_fold_batch(h, c.data(), z.data(), gamma.data(), y.data(), w.data(), 1, k, &verdict, &st);
        rc = e != 0 ? failed(st) : verdict_of(verdict);
    }
    gwb_kzg_free(h);
    return rc;
}
