// Host build of r1cs/g2_subgroup_gfx950.hpp for tests/test_g2_subgroup_host.py (g++ -fsanitize=address,undefined).  Reads
// lines from stdin, every number 64 hexadecimal digits (canonical, most significant digit first):
//   S x0 x1 y0 y1          -> "S <g2_in_subgroup> <g2_in_subgroup_by_order> <on the twist>"   ((0, 0) is infinity)
//   P x0 x1 y0 y1 l0 l1    -> "P x0 x1 y0 y1": psi of the point given to g2_psi as the projective XYZZ point
//                             (x l^2, y l^3, l^2, l^3), l = l0 + l1 u != 0, made affine again
#include <stdio.h>
#include <string.h>

#include <string>

#include "../../circom-witnesscalc_amd/r1cs/g2_subgroup_gfx950.hpp"

using namespace cwc_g16;

static bool parse_hex(const char* s, Fq& out) {
    if (strlen(s) != 64) return false;
    for (int i = 0; i < 8; ++i) out.v[i] = 0;
    for (int i = 0; i < 64; ++i) {
        const char c = s[i];
        const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
        if (d < 0) return false;
        const int bit = 4 * (63 - i);
        out.v[bit >> 5] |= (uint32_t)d << (bit & 31);
    }
    return true;
}

static std::string hex_of(const Fq& mont) {
    const Fq c = fq_from_mont(mont);
    char buf[65];
    for (int i = 0; i < 8; ++i) snprintf(buf + 8 * i, 9, "%08x", c.v[7 - i]);
    return buf;
}

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        char kind = 0, w[6][80];
        const int got = sscanf(line, " %c %79s %79s %79s %79s %79s %79s", &kind, w[0], w[1], w[2], w[3], w[4], w[5]);
        const int need = kind == 'S' ? 4 : kind == 'P' ? 6 : -1;
        Fq v[6];
        if (need < 0 || got != need + 1) {
            fprintf(stderr, "bad line: %s", line);
            return 1;
        }
        for (int i = 0; i < need; ++i) {
            if (!parse_hex(w[i], v[i]) || !cwc::u256_lt(v[i], fq_p())) {
                fprintf(stderr, "bad number: %s\n", w[i]);
                return 1;
            }
            v[i] = fq_to_mont(v[i]);
        }
        const Affine<Fq2T> p{Fq2{v[0], v[1]}, Fq2{v[2], v[3]}};
        if (kind == 'S') {
            const bool on = affine_is_inf(p) || on_curve<Fq2T>(p, twist_b());
            printf("S %d %d %d\n", g2_in_subgroup(p) ? 1 : 0, g2_in_subgroup_by_order(p) ? 1 : 0, on ? 1 : 0);
        } else {
            const Fq2 l{v[4], v[5]}, l2 = fq2_sqr(l), l3 = fq2_mul(l2, l);
            const Xyzz<Fq2T> in{fq2_mul(p.x, l2), fq2_mul(p.y, l3), l2, l3};
            const Affine<Fq2T> o = xyzz_to_affine(g2_psi(in));
            printf("P %s %s %s %s\n", hex_of(o.x.c0).c_str(), hex_of(o.x.c1).c_str(), hex_of(o.y.c0).c_str(), hex_of(o.y.c1).c_str());
        }
    }
    return 0;
}
