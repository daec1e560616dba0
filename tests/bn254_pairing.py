"""Plain-Python BN254 optimal ate pairing, the oracle of the Groth16 verifier's tests (include/graph_witness_groth16_verify.h).

Deliberately not the device's representation: Fq12 here is the flat Fq[w]/(w^12 - 18 w^6 + 82), the twisted G2 point is
mapped into E(Fq12) and the Miller loop runs on affine points of E(Fq12) with slopes in Fq12 (polynomial inverses), and the
final exponentiation is one plain power by (q^12 - 1) / r.  The device's tower Fq12 = Fq6[w]/(w^2 - v), Fq6 = Fq2[v]/(v^3 -
(9 + u)), Fq2 = Fq[u]/(u^2 + 1) meets it through an explicit map (u = w^6 - 9, v = w^2): to_tower / from_tower, and gt_bytes
(384 bytes, 12 canonical little-endian Fq values in the order c0.b0.a0, c0.b0.a1, c0.b1.a0, ..., c1.b2.a1)."""
from tests import groth16_fixtures as GF

Q, R = GF.Q, GF.R
X = 4965661367192848881          # the BN parameter
ATE = 6 * X + 2                  # Miller loop length
FINAL_EXP = (Q ** 12 - 1) // R
MOD = [82, 0, 0, 0, 0, 0, -18, 0, 0, 0, 0, 0]  # w^12 = 18 w^6 - 82


# -- flat Fq12: tuples of 12 ints --------------------------------------------------------------------------------------------
def f12(c0=0):
    return (c0 % Q,) + (0,) * 11


ONE = f12(1)


def add(a, b):
    return tuple((x + y) % Q for x, y in zip(a, b))


def sub(a, b):
    return tuple((x - y) % Q for x, y in zip(a, b))


def neg(a):
    return tuple(-x % Q for x in a)


def scale(a, k):
    return tuple(x * k % Q for x in a)


def mul(a, b):
    t = [0] * 23
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                t[i + j] += x * y
    for k in range(22, 11, -1):  # w^k = w^(k-12) (18 w^6 - 82)
        c, t[k] = t[k], 0
        if c:
            t[k - 6] += 18 * c
            t[k - 12] -= 82 * c
    return tuple(x % Q for x in t[:12])


def power(a, e):
    acc = ONE
    for bit in bin(e)[2:] if e > 0 else "":
        acc = mul(acc, acc)
        if bit == "1":
            acc = mul(acc, a)
    return acc


def _deg(p):
    d = len(p) - 1
    while d and p[d] == 0:
        d -= 1
    return d


def inv(a):
    """extended Euclid over Fq[w] against the modulus polynomial"""
    lm, hm = [1] + [0] * 12, [0] * 13
    low, high = list(a) + [0], [m % Q for m in MOD] + [1]
    assert any(a), "inverse of zero"
    while _deg(low):
        r = [0] * 13  # high / low
        h = list(high)
        dl = _deg(low)
        il = pow(low[dl], Q - 2, Q)
        for d in range(_deg(h) - dl, -1, -1):
            c = h[d + dl] * il % Q
            r[d] = c
            for i in range(dl + 1):
                h[d + i] = (h[d + i] - c * low[i]) % Q
        nm = list(hm)
        for i in range(13):
            for j in range(13 - i):
                nm[i + j] = (nm[i + j] - lm[i] * r[j]) % Q
        lm, low, hm, high = nm, h, lm, low
    il = pow(low[0], Q - 2, Q)
    return tuple(x * il % Q for x in lm[:12])


# -- E(Fq12): affine (x, y) or None -------------------------------------------------------------------------------------------
def _double(p):
    x, y = p
    m = mul(scale(mul(x, x), 3), inv(scale(y, 2)))
    nx = sub(mul(m, m), scale(x, 2))
    return nx, sub(mul(m, sub(x, nx)), y)


def _add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    if p1[0] == p2[0]:
        return _double(p1) if p1[1] == p2[1] else None
    m = mul(sub(p2[1], p1[1]), inv(sub(p2[0], p1[0])))
    nx = sub(sub(mul(m, m), p1[0]), p2[0])
    return nx, sub(mul(m, sub(p1[0], nx)), p1[1])


def _line(p1, p2, t):
    """the line through p1 and p2 (tangent if equal) evaluated at t"""
    (x1, y1), (x2, y2), (xt, yt) = p1, p2, t
    if x1 != x2:
        m = mul(sub(y2, y1), inv(sub(x2, x1)))
    elif y1 == y2:
        m = mul(scale(mul(x1, x1), 3), inv(scale(y1, 2)))
    else:
        return sub(xt, x1)
    return sub(mul(m, sub(xt, x1)), sub(yt, y1))


def fq2_embed(a):
    """a0 + a1 u -> flat (u = w^6 - 9)"""
    c = [0] * 12
    c[0], c[6] = (a[0] - 9 * a[1]) % Q, a[1] % Q
    return tuple(c)


W2, W3 = tuple(1 if i == 2 else 0 for i in range(12)), tuple(1 if i == 3 else 0 for i in range(12))


def untwist(q):
    """affine G2 point on y^2 = x^3 + 3 / (9 + u) -> E(Fq12): (x w^2, y w^3)"""
    return None if q is None else (mul(fq2_embed(q[0]), W2), mul(fq2_embed(q[1]), W3))


def frob(a):
    return power(a, Q)


def miller(p, q):
    """f_{6x+2,Q}(P) times the two final lines (affine P in G1, Q on the twist; None = infinity)"""
    if p is None or q is None:
        return ONE
    P = (f12(p[0]), f12(p[1]))
    Qt = untwist(q)
    T, f = Qt, ONE
    for i in range(ATE.bit_length() - 2, -1, -1):
        f = mul(mul(f, f), _line(T, T, P))
        T = _double(T)
        if (ATE >> i) & 1:
            f = mul(f, _line(T, Qt, P))
            T = _add(T, Qt)
    q1 = (frob(Qt[0]), frob(Qt[1]))
    nq2 = (frob(q1[0]), neg(frob(q1[1])))
    f = mul(f, _line(T, q1, P))
    T = _add(T, q1)
    return mul(f, _line(T, nq2, P))


def final_exp(f):
    return power(f, FINAL_EXP)


def pairing(p, q):
    """e(P, Q) for affine P in G1 and Q in G2 (twist coordinates, Fq2 tuples); None = infinity"""
    return final_exp(miller(p, q))


# -- the device's tower -------------------------------------------------------------------------------------------------------
# tower position of w^i's Fq2 coefficient (index into the 6 Fq2 values c0.b0, c0.b1, c0.b2, c1.b0, c1.b1, c1.b2)
_POS = {0: 0, 1: 3, 2: 1, 3: 4, 4: 2, 5: 5}


def to_tower(a):
    """flat -> [12] Fq in the device order c0.b0.a0, c0.b0.a1, c0.b1.a0, ..., c1.b2.a1"""
    out = [0] * 12
    for i in range(6):
        b = a[i + 6]
        k = _POS[i]
        out[2 * k], out[2 * k + 1] = (a[i] + 9 * b) % Q, b
    return out


def from_tower(t):
    c = [0] * 12
    for i in range(6):
        k = _POS[i]
        a0, a1 = t[2 * k], t[2 * k + 1]
        c[i], c[i + 6] = (a0 - 9 * a1) % Q, a1 % Q
    return tuple(c)


def gt_bytes(a):
    return b"".join(x.to_bytes(32, "little") for x in to_tower(a))


def gt_from_bytes(b):
    return from_tower([int.from_bytes(b[32 * k:32 * k + 32], "little") for k in range(12)])


def tower_mul(s, t):
    """schoolbook product in the tower itself (for the isomorphism test): [12] Fq x [12] Fq -> [12] Fq"""
    def m2(a, b):
        return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)

    def a2(a, b):
        return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)

    xi = (9, 1)

    def m6(a, b):
        c = [(0, 0)] * 5
        for i in range(3):
            for j in range(3):
                c[i + j] = a2(c[i + j], m2(a[i], b[j]))
        return [a2(c[0], m2(xi, c[3])), a2(c[1], m2(xi, c[4])), c[2]]

    def split(x):
        f2 = [(x[2 * k], x[2 * k + 1]) for k in range(6)]
        return f2[:3], f2[3:]

    (s0, s1), (t0, t1) = split(s), split(t)
    c0 = [a2(x, y) for x, y in zip(m6(s0, t0), _mul_v(m6(s1, t1), m2, xi))]
    c1 = [a2(x, y) for x, y in zip(m6(s0, t1), m6(s1, t0))]
    return [c for pair in c0 + c1 for c in pair]


def _mul_v(a, m2, xi):
    """(a0 + a1 v + a2 v^2) v = xi a2 + a0 v + a1 v^2"""
    return [m2(xi, a[2]), a[0], a[1]]


# -- G2 helpers for the tests --------------------------------------------------------------------------------------------------
def twist_point_outside_subgroup(rnd):
    """a point on the twist y^2 = x^3 + B2 that is not in the order-r subgroup: y solved at a random x, no cofactor clearing"""
    F2 = GF.Fq2
    while True:
        x = (rnd.randrange(Q), rnd.randrange(Q))
        rhs = F2.add(F2.mul(F2.mul(x, x), x), GF.B2)
        y = fq2_sqrt(rhs)
        if y is None:
            continue
        p = (x, y)
        assert GF.G2.on_curve(p)
        if not GF.G2.is_inf(GF.G2.mul(p, R)):
            return p


def fq2_sqrt(a):
    """a square root in Fq2 (q = 3 mod 4), or None"""
    F2 = GF.Fq2
    if a == (0, 0):
        return (0, 0)
    # norm must be a square in Fq
    n = (a[0] * a[0] + a[1] * a[1]) % Q
    s = pow(n, (Q + 1) // 4, Q)
    if s * s % Q != n:
        return None
    for sg in (s, -s % Q):
        t = (a[0] + sg) * pow(2, Q - 2, Q) % Q
        x0 = pow(t, (Q + 1) // 4, Q)
        if x0 * x0 % Q != t or x0 == 0:
            continue
        x1 = a[1] * pow(2 * x0, Q - 2, Q) % Q
        if F2.mul((x0, x1), (x0, x1)) == (a[0] % Q, a[1] % Q):
            return (x0, x1)
    return None
