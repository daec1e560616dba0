// Membership of a point of BN254's twist in G2, the subgroup of order r, without the multiplication by r.
//
// The twist E'(Fq2): y^2 = x^3 + 3 / (9 + u) has order r c2, c2 = 2q - r = 10069 * 5864401 * ..., so a point on the curve can
// carry a component of small order.  With x = 4965661367192848881 (BN_X) and psi the untwist-Frobenius-twist endomorphism
//   psi(x, y) = (conj(x) xi^((q - 1) / 3), conj(y) xi^((q - 1) / 2)),   xi = 9 + u   (g2_frob1 of fq12_gfx950.hpp),
// a point P of E'(Fq2) lies in G2 if and only if
//   [x + 1] P + psi([x] P) + psi^2([x] P) = psi^3([2x] P)
// (Dai, Lin, Zhao, Zhou, "Fast subgroup membership testings for G1, G2 and GT on pairing-friendly curves"; gnark-crypto's
// bn254 check).  On G2 psi acts as multiplication by q, and the equation is r | (x + 1) + x q + x q^2 - 2x q^3 there; the paper
// shows that no point outside G2 satisfies it.  Cost: one 63-bit double-and-add (62 doublings, 27 mixed additions), one more
// mixed addition, two additions, one doubling, three psi (psi^3([2x] P) = 2 psi(psi^2([x] P))) and one comparison, against
// 254 doublings and 127 additions for [r] P.
//
// psi on XYZZ coordinates (x = X / ZZ, y = Y / ZZZ): conjugation is a field automorphism, so conj(x) = conj(X) / conj(ZZ) and
// conj(y) = conj(Y) / conj(ZZZ), and conj(ZZ)^3 = conj(ZZZ)^2 still holds; the two constants scale X and Y alone.
//
// Host and device share this code (FRD), as the rest of fq_gfx950.hpp.  Montgomery form throughout.
#pragma once
#include "fq12_gfx950.hpp"

namespace cwc_g16 {

FRD Xyzz<Fq2T> g2_psi(const Xyzz<Fq2T>& p) {
    return Xyzz<Fq2T>{fq2_mul(fq2_conj(p.X), frob1_2()), fq2_mul(fq2_conj(p.Y), frob1_3()), fq2_conj(p.ZZ), fq2_conj(p.ZZZ)};
}

// [BN_X] p for an affine p other than infinity: double-and-add from the bit below the top one, the bits a compile-time constant
FRD Xyzz<Fq2T> g2_mul_x(const Affine<Fq2T>& p) {
    static_assert((BN_X >> 62) == 1ull, "x has 63 bits");
    Xyzz<Fq2T> acc{p.x, p.y, fq2_one(), fq2_one()};
    for (int b = 61; b >= 0; --b) {
        acc = xyzz_dbl(acc);
        if ((BN_X >> b) & 1ull) acc = xyzz_add_affine(acc, p);
    }
    return acc;
}

// the same point?  By cross-multiplication: X1 ZZ2 = X2 ZZ1 and Y1 ZZZ2 = Y2 ZZZ1; infinity equals infinity alone.
FRD bool g2_xyzz_eq(const Xyzz<Fq2T>& a, const Xyzz<Fq2T>& b) {
    const bool ia = xyzz_is_inf(a), ib = xyzz_is_inf(b);
    const bool same = cwc::both(Fq2T::eq(fq2_mul(a.X, b.ZZ), fq2_mul(b.X, a.ZZ)), Fq2T::eq(fq2_mul(a.Y, b.ZZZ), fq2_mul(b.Y, a.ZZZ)));
    return cwc::either(cwc::both(ia, ib), cwc::both(cwc::both(!ia, !ib), same));
}

// p on the twist (not checked here), (0, 0) = infinity: is it in the subgroup of order r?
FRD bool g2_in_subgroup(const Affine<Fq2T>& p) {
    if (affine_is_inf(p)) return true;
    Xyzz<Fq2T> t = g2_mul_x(p);                      // [x] P
    Xyzz<Fq2T> lhs = xyzz_add_affine(t, p);          // [x + 1] P
    t = g2_psi(t);
    lhs = xyzz_add(lhs, t);                          // + psi([x] P)
    t = g2_psi(t);
    lhs = xyzz_add(lhs, t);                          // + psi^2([x] P)
    t = xyzz_dbl(g2_psi(t));                         // psi^3([2x] P)
    return g2_xyzz_eq(lhs, t);
}

// the rule this replaces where it is used, and its cross-check: [r] P = O by the 254-bit double-and-add
FRD bool g2_in_subgroup_by_order(const Affine<Fq2T>& p) {
    if (affine_is_inf(p)) return true;
    return xyzz_is_inf(xyzz_mul(from_affine(p), cwc::fr_p()));
}

}  // namespace cwc_g16
