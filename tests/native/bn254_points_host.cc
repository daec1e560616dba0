// Host build of r1cs/bn254_points_gfx950.hpp for tests/test_bn254_points_host.py (g++ -fsanitize=address,undefined): the code the
// device kernels decode and encode points with.  Reads lines from stdin; <group> is 1 or 2, <form> is m (Montgomery) or c
// (canonical), <bytes> the stored point in hexadecimal, two digits per byte in memory order (64 bytes for G1, 128 for G2).  The
// bytes are handed over at an odd address, as a mapped file may hold them.
//   F <group> <form> <bytes>  -> "F <point_fault>"  (0 coordinate, 1 curve, 3 none)
//   R <group> <form> <bytes>  -> "R <in range> <bytes>": get_coords, from_affine, xyzz_to_affine, put_coords in the same form
//   B                         -> "B <curve_b<G1>() is Montgomery 3> <curve_b<G2>() is 3 / (9 + u) by fq2_inv>"
//   G                         -> "G <g1 on its curve> <g2 on its curve> <g2_in_subgroup> <g1 canonical bytes> <g2 canonical bytes>"
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../circom-witnesscalc_amd/r1cs/g2_subgroup_gfx950.hpp"

using namespace cwc_g16;

static bool parse_bytes(const char* s, uint8_t* out, size_t n) {
    if (strlen(s) != 2 * n) return false;
    for (size_t i = 0; i < 2 * n; ++i) {
        const char c = s[i];
        const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
        if (d < 0) return false;
        out[i / 2] = (uint8_t)(i % 2 ? out[i / 2] | d : d << 4);
    }
    return true;
}

static std::string hex_of(const uint8_t* p, size_t n) {
    std::string s(2 * n, '0');
    for (size_t i = 0; i < n; ++i) snprintf(&s[2 * i], 3, "%02x", p[i]);
    return s;
}

template <class T>
static void point_line(char kind, const uint8_t* in, bool canonical) {
    constexpr size_t N = sizeof(Affine<T>);
    if (kind == 'F') {
        printf("F %u\n", (unsigned)point_fault<T>(in, canonical));
        return;
    }
    Affine<T> a;
    const bool ok = get_coords<T>(in, canonical, a.x, a.y);
    const Affine<T> b = xyzz_to_affine(from_affine(a));
    std::vector<uint8_t> out(N + 1);
    put_coords<T>(out.data() + 1, b.x, b.y, canonical);
    printf("R %d %s\n", ok ? 1 : 0, hex_of(out.data() + 1, N).c_str());
}

int main() {
    static char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        char kind = 0, form = 0;
        static char hex[512];
        unsigned group = 0;
        const int got = sscanf(line, " %c %u %c %300s", &kind, &group, &form, hex);
        if (kind == 'B' && got == 1) {
            const Fq2 xi{fq_to_mont(Fq{{9, 0, 0, 0, 0, 0, 0, 0}}), fq_one()};
            const Fq three = fq_to_mont(Fq{{3, 0, 0, 0, 0, 0, 0, 0}});
            const Fq2 i = fq2_inv(xi), b2{fq_mul(i.c0, three), fq_mul(i.c1, three)};
            printf("B %d %d\n", cwc::u256_eq(curve_b<G1>(), three) ? 1 : 0, Fq2T::eq(curve_b<G2>(), b2) ? 1 : 0);
        } else if (kind == 'G' && got == 1) {
            const A1 g1 = g1_generator();
            const A2 g2 = g2_generator();
            uint8_t b1[sizeof(A1)], b2[sizeof(A2)];
            put_coords<G1>(b1, g1.x, g1.y, true);
            put_coords<G2>(b2, g2.x, g2.y, true);
            printf("G %d %d %d %s %s\n", on_curve<G1>(g1, curve_b<G1>()) ? 1 : 0, on_curve<G2>(g2, curve_b<G2>()) ? 1 : 0, g2_in_subgroup(g2) ? 1 : 0,
                   hex_of(b1, sizeof b1).c_str(), hex_of(b2, sizeof b2).c_str());
        } else if ((kind == 'F' || kind == 'R') && got == 4 && (group == 1 || group == 2) && (form == 'm' || form == 'c')) {
            const size_t n = group == 1 ? sizeof(A1) : sizeof(A2);
            std::vector<uint8_t> buf(1 + n);  // exactly the point: a read past it is the sanitizer's to find
            if (!parse_bytes(hex, buf.data() + 1, n)) {
                fprintf(stderr, "bad bytes: %s", line);
                return 1;
            }
            if (group == 1)
                point_line<G1>(kind, buf.data() + 1, form == 'c');
            else
                point_line<G2>(kind, buf.data() + 1, form == 'c');
        } else {
            fprintf(stderr, "bad line: %s", line);
            return 1;
        }
    }
    return 0;
}
