"""Points of BN254's twist E'(Fq2): y^2 = x^3 + 3 / (9 + u) for the G2 subgroup-membership tests, on the plain-Python curve of
groth16_fixtures: the classes that a membership test has to tell apart, psi (the untwist-Frobenius-twist endomorphism) and the
criterion [x + 1] P + psi([x] P) + psi^2([x] P) = psi^3([2x] P), restated here from the paper's formulas on affine points and
Jacobian sums, independently of r1cs/g2_subgroup_gfx950.hpp.  The twist has order r c2 with c2 = 2q - r = 10069 * 5864401 * ...;
the reference verdict is [r] P = O."""
import functools
import random

from tests import bn254_pairing as BP
from tests import groth16_fixtures as GF

Q, R = GF.Q, GF.R
X = BP.X
C2 = 2 * Q - R
SMALL = (10069, 5864401)
assert C2 % SMALL[0] == 0 and C2 % SMALL[1] == 0
F2, G2 = GF.Fq2, GF.G2
CLASSES = ("random_twist", "cofactor_cleared", "order_10069", "order_5864401", "g2_plus_torsion", "r_times")


def fq2_pow(a, e):
    acc = F2.one
    for bit in bin(e)[2:]:
        acc = F2.mul(acc, acc)
        if bit == "1":
            acc = F2.mul(acc, a)
    return acc


XI = (9, 1)
PSI_X = fq2_pow(XI, (Q - 1) // 3)
PSI_Y = fq2_pow(XI, (Q - 1) // 2)


def conj(a):
    return (a[0], -a[1] % Q)


def psi(p):
    """affine point (or None) -> psi of it"""
    if p is None:
        return None
    return (F2.mul(conj(p[0]), PSI_X), F2.mul(conj(p[1]), PSI_Y))


def in_g2_by_order(p):
    return G2.is_inf(G2.mul(p, R))


def in_g2_by_psi(p):
    """[x + 1] P + psi([x] P) + psi^2([x] P) == psi^3([2x] P), on affine points"""
    if p is None:
        return True
    xp = G2.to_affine(G2.mul(p, X))
    lhs = G2.add(G2.add(G2.mul(p, X + 1), G2.jac(psi(xp))), G2.jac(psi(psi(xp))))
    rhs = psi(psi(psi(G2.to_affine(G2.mul(p, 2 * X)))))
    return G2.to_affine(lhs) == rhs


def in_g2_by_psi_short(p):
    """the two-term criterion psi(P) == [6 x^2] P"""
    return p is None or psi(p) == G2.to_affine(G2.mul(p, 6 * X * X))


def random_twist_point(rnd):
    """any point of the twist: y solved at a random x"""
    while True:
        x = (rnd.randrange(Q), rnd.randrange(Q))
        y = BP.fq2_sqrt(F2.add(F2.mul(F2.mul(x, x), x), GF.B2))
        if y is not None:
            if rnd.random() < 0.5:
                y = F2.neg(y)
            assert G2.on_curve((x, y))
            return (x, y)


def exact_order(rnd, ell):
    """a point of exact prime order ell | c2"""
    while True:
        p = G2.to_affine(G2.mul(random_twist_point(rnd), R * C2 // ell))
        if p is not None:
            assert G2.is_inf(G2.mul(p, ell))
            return p


def point_of(cls, rnd):
    if cls == "random_twist":
        return random_twist_point(rnd)
    if cls == "cofactor_cleared":
        return G2.to_affine(G2.mul(random_twist_point(rnd), C2))
    if cls == "order_10069":
        return exact_order(rnd, SMALL[0])
    if cls == "order_5864401":
        return exact_order(rnd, SMALL[1])
    if cls == "g2_plus_torsion":
        g = G2.gen_mul_jac(rnd.randrange(1, R))
        return G2.to_affine(G2.add(g, G2.jac(exact_order(rnd, SMALL[0]))))
    if cls == "r_times":
        return G2.to_affine(G2.mul(random_twist_point(rnd), R))
    raise ValueError(cls)


@functools.lru_cache(maxsize=None)
def samples(per_class, seed=2024):
    """[(class, affine point, in G2?)], `per_class` of each class, made once per process; the verdict is [r] P = O"""
    rnd = random.Random(seed)
    out = []
    for cls in CLASSES:
        for _ in range(per_class):
            p = point_of(cls, rnd)
            out.append((cls, p, in_g2_by_order(p)))
    return tuple(out)


def canonical_bytes(p):
    """128 canonical little-endian bytes (zero = infinity)"""
    return bytes(128) if p is None else b"".join(v.to_bytes(32, "little") for v in (p[0][0], p[0][1], p[1][0], p[1][1]))
