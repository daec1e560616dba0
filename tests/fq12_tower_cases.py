"""Case lists and expected values of the pairing-tower tests (tests/test_fq12_tower_host.py on the CPU, tests/test_gpu_fq12_tower.py
on an MI355X): operand records for the primitives of r1cs/fq12_gfx950.hpp, in the section format of tests/native/fq12_tower.hip
(record layouts: tests/native/fq12_tower_ops.hpp), and what each record must give.

The oracle is tests/bn254_pairing.py's flat Fq12 = Fq[w]/(w^12 - 18 w^6 + 82) (mul, inv, power, to_tower / from_tower) and
groth16_fixtures.Fq2 / Curve with Python integers; nothing here comes from the code under test.  Fq6 values are embedded with
c1 = 0, the Frobenius maps are power(x, Q^k), cyclotomic squaring is mul(a, a), the easy part power(f, (Q^6 - 1)(Q^2 + 1)), the
hard part power(g, (Q^4 - Q^2 + 1) / R), that exponent itself.  xi is the Fq2 element (9, 1), v the flat element w^2.  A line of a
Miller step is defined up to an Fq2 factor: with s the tangent or chord slope at the affine T, (a, b, c) must be proportional to
(1, -s, s x_T - y_T) with a != 0, and T after the step is compared as (X / Z, Y / Z) with the Curve result.

Operand classes, at every level of the tower and in every operand position: zero, one, -1, each basis coefficient alone (1, q - 1,
a random value), elements of the subfields embedded, c0 = 0, all coefficients q - 1, Fq2 operands with c0 + c1 = q, c0 = c1 and
c0 = -c1, random elements.  A case is (group, special, record bytes, expected, name): `group` names the wave it shares in the
uniform arrangement, `special` whether it sits at lanes 0, 63 and the even lanes of the mixed waves."""
import functools
import os
import random
import subprocess

import numpy as np

from tests import bn254_pairing as BP
from tests import groth16_fixtures as GF

Q, R, MONT = GF.Q, GF.R, GF.MONT
MONT_INV = pow(MONT, -1, Q)
F2 = GF.Fq2
XI = (9, 1)
GUARD = 64   # guard records after every section's results (fq12_tower_ops.hpp)
EASY_EXP = (Q ** 6 - 1) * (Q ** 2 + 1)
HARD_EXP = (Q ** 4 - Q ** 2 + 1) // R
assert (Q ** 4 - Q ** 2 + 1) % R == 0 and EASY_EXP * HARD_EXP == BP.FINAL_EXP

_NAMES = ("FQ_HALF FQ2_HALF FQ2_MUL FQ2_SQR FQ2_INV FQ2_CONJ FQ2_MUL_FQ FQ2_MUL_XI FQ6_MUL FQ6_MUL_01 FQ6_MUL_FQ2 FQ6_MUL_V FQ6_INV "
          "FQ12_MUL FQ12_SQR FQ12_INV FQ12_CONJ FQ12_MUL_LINE FQ12_MUL_LINE_AT FQ12_FROB FQ12_CSQ FINAL_EASY FINAL_HARD "
          "G2_DBL_STEP G2_ADD_STEP G2_FROB1 G2_NEG_FROB2 MILLER_STEP").split()
OP = {n: i + 1 for i, n in enumerate(_NAMES)}
IN_WORDS = dict(FQ_HALF=8, FQ2_HALF=16, FQ2_MUL=32, FQ2_SQR=16, FQ2_INV=16, FQ2_CONJ=16, FQ2_MUL_FQ=24, FQ2_MUL_XI=16, FQ6_MUL=96,
                FQ6_MUL_01=80, FQ6_MUL_FQ2=64, FQ6_MUL_V=48, FQ6_INV=48, FQ12_MUL=192, FQ12_SQR=96, FQ12_INV=96, FQ12_CONJ=96,
                FQ12_MUL_LINE=144, FQ12_MUL_LINE_AT=160, FQ12_FROB=97, FQ12_CSQ=96, FINAL_EASY=96, FINAL_HARD=96, G2_DBL_STEP=48,
                G2_ADD_STEP=80, G2_FROB1=32, G2_NEG_FROB2=32, MILLER_STEP=81)
OUT_WORDS = {n: 8 if n == "FQ_HALF" else 16 if n.startswith("FQ2_") else 48 if n.startswith("FQ6_") else 32 if "FROB" in n and n.startswith("G2")
             else 96 for n in _NAMES}
FAMILIES = {"fq2": _NAMES[:8], "fq6": _NAMES[8:13], "fq12": _NAMES[13:20], "final": _NAMES[20:23], "steps": _NAMES[23:]}
N_RANDOM = 4


# -- encoding ------------------------------------------------------------------------------------------------------------------
def enc(vals):
    """canonical Fq values -> bytes of their Montgomery limbs"""
    return b"".join((v * MONT % Q).to_bytes(32, "little") for v in vals)


def word(k):
    return int(k).to_bytes(4, "little")


def dec(words, what=""):
    """u32 words -> canonical Fq values; every raw coefficient must be below q"""
    raw = np.ascontiguousarray(words, dtype="<u4").tobytes()
    out = []
    for i in range(len(raw) // 32):
        c = int.from_bytes(raw[32 * i:32 * i + 32], "little")
        assert c < Q, "%s: coefficient %d is not reduced" % (what, i)
        out.append(c * MONT_INV % Q)
    return out


# -- the oracle's additions -------------------------------------------------------------------------------------------------------
def flat(t):
    """tower coefficients of an Fq, Fq2, Fq6 or Fq12 element (1, 2, 6 or 12 values) -> flat Fq12"""
    return BP.from_tower(list(t) + [0] * (12 - len(t)))


def tower(a, width=12):
    t = BP.to_tower(a)
    assert not any(t[width:]), "the value left its subfield"
    return t[:width]


def conj12(a):
    """w -> -w, the automorphism of Fq12 over Fq6 (= power(a, Q^6), asserted once by the host test)"""
    return tuple(-c % Q if i & 1 else c for i, c in enumerate(a))


def line_flat(l0, l1, l3):
    """l0 + l1 w + l3 w^3"""
    W1 = tuple(1 if i == 1 else 0 for i in range(12))
    return BP.add(BP.add(BP.fq2_embed(l0), BP.mul(BP.fq2_embed(l1), W1)), BP.mul(BP.fq2_embed(l3), BP.W3))


@functools.lru_cache(maxsize=None)
def easy_of(a):
    return BP.power(a, EASY_EXP)


W2_INV, W3_INV = BP.inv(BP.W2), BP.inv(BP.W3)


def twist_frob(p, k):
    """pi^k of an affine twist point: coordinate-wise power(., Q^k) of the untwisted point, mapped back"""
    ux, uy = BP.untwist(p)
    x = tower(BP.mul(BP.power(ux, Q ** k), W2_INV), 2)
    y = tower(BP.mul(BP.power(uy, Q ** k), W3_INV), 2)
    return (tuple(x), tuple(y))


# -- operand classes --------------------------------------------------------------------------------------------------------------
def unit(width, i, v):
    return [v if j == i else 0 for j in range(width)]


def rand_el(rnd, width):
    return [rnd.randrange(1, Q) for _ in range(width)]


def element_classes(width, rnd):
    """[(group, special, name, coefficients)] of an element of `width` Fq coefficients in tower order"""
    out = [("units", True, "zero", [0] * width), ("units", True, "one", unit(width, 0, 1)), ("units", True, "minus one", unit(width, 0, Q - 1))]
    for i in range(width):
        for name, v in (("1", 1), ("q - 1", Q - 1), ("random", rnd.randrange(2, Q - 1))):
            out.append(("basis", True, "basis %d = %s" % (i, name), unit(width, i, v)))
    subs = [s for s in (1, 2, 6) if s < width]
    for s in subs:
        out.append(("subfield", True, "in Fq%s" % ("" if s == 1 else s), rand_el(rnd, s) + [0] * (width - s)))
    if width == 12:
        out.append(("subfield", True, "c0 = 0", [0] * 6 + rand_el(rnd, 6)))
    out.append(("units", True, "all q - 1", [Q - 1] * width))
    if width == 2:
        a, b, c = (rnd.randrange(1, Q) for _ in range(3))
        out += [("fq2 forms", True, "c0 + c1 = q", [a, Q - a]), ("fq2 forms", True, "c0 = c1", [b, b]), ("fq2 forms", True, "c0 = -c1", [Q - c, c])]
    out += [("random", False, "random", rand_el(rnd, width)) for _ in range(N_RANDOM)]
    assert len(out) == 4 + 3 * width + len(subs) + (width == 12) + 3 * (width == 2) + N_RANDOM
    return out


CORE = ("units", "subfield", "fq2 forms")


def pair_classes(A, B, rnd):
    """operand pairs: every pair of the core classes (units, subfields, Fq2 forms), every class once in each position beside a
    random partner, and basis elements against basis elements"""
    gen_a, gen_b = [c for c in A if not c[1]], [c for c in B if not c[1]]
    core_a, core_b = [c for c in A if c[0] in CORE], [c for c in B if c[0] in CORE]
    basis_a, basis_b = [c for c in A if c[0] == "basis"], [c for c in B if c[0] == "basis"]
    out = [("special x special", True, a, b) for a in core_a for b in core_b]
    out += [("special x generic" if a[1] else "generic", a[1], a, rnd.choice(gen_b)) for a in A]
    out += [("generic x special" if b[1] else "generic", b[1], rnd.choice(gen_a), b) for b in B]
    out += [("basis x basis", True, a, basis_b[(5 * i + 3) % len(basis_b)]) for i, a in enumerate(basis_a)]
    assert len(out) == len(core_a) * len(core_b) + len(A) + len(B) + len(basis_a)
    return [(g, s, "%s x %s" % (a[2], b[2]), a[3], b[3]) for g, s, a, b in out]


def fq2_mul_t(a, b):
    return list(F2.mul(tuple(a), tuple(b)))


# -- the case lists, per family -----------------------------------------------------------------------------------------------------
def fq2_cases():
    rnd = random.Random(201)
    half = [("units", True, "raw %s" % n, m) for n, m in (("0", 0), ("1", 1), ("2", 2), ("q - 1", Q - 1), ("q - 2", Q - 2))]
    # an odd limb value whose sum with q carries through j whole words
    half += [("carry", True, "raw -q mod 2^%d" % (32 * j), (1 << (32 * j)) - Q % (1 << (32 * j))) for j in range(1, 8)]
    half += [("random odd", False, "raw odd", rnd.randrange(Q) | 1) for _ in range(N_RANDOM)]
    half += [("random even", False, "raw even", rnd.randrange(Q) & ~1) for _ in range(N_RANDOM)]
    assert len(half) == 12 + 2 * N_RANDOM and all(m < Q for *_, m in half)
    inv2 = pow(2, Q - 2, Q)
    ops = {"FQ_HALF": [(g, s, enc([m * MONT_INV % Q]), [m * MONT_INV * inv2 % Q], n) for g, s, n, m in half]}
    E2, E1 = element_classes(2, rnd), element_classes(1, rnd)
    un = {"FQ2_HALF": lambda a: [a[0] * inv2 % Q, a[1] * inv2 % Q], "FQ2_SQR": lambda a: fq2_mul_t(a, a),
          "FQ2_INV": lambda a: list(F2.inv(tuple(a))) if any(a) else [0, 0], "FQ2_CONJ": lambda a: [a[0], -a[1] % Q],
          "FQ2_MUL_XI": lambda a: fq2_mul_t(a, XI)}
    for op, fn in un.items():
        ops[op] = [(g, s, enc(a), fn(a), n) for g, s, n, a in E2]
    ops["FQ2_MUL"] = [(g, s, enc(a + b), fq2_mul_t(a, b), n) for g, s, n, a, b in pair_classes(E2, E2, rnd)]
    ops["FQ2_MUL_FQ"] = [(g, s, enc(a + b), [a[0] * b[0] % Q, a[1] * b[0] % Q], n) for g, s, n, a, b in pair_classes(E2, E1, rnd)]
    return ops


def fq6_cases():
    rnd = random.Random(202)
    E6, E2 = element_classes(6, rnd), element_classes(2, rnd)

    def mul6(a, b):
        return tower(BP.mul(flat(a), flat(b)), 6)

    ops = {"FQ6_MUL": [(g, s, enc(a + b), mul6(a, b), n) for g, s, n, a, b in pair_classes(E6, E6, rnd)],
           "FQ6_MUL_FQ2": [(g, s, enc(a + b), mul6(a, b), n) for g, s, n, a, b in pair_classes(E6, E2, rnd)],
           "FQ6_MUL_V": [(g, s, enc(a), tower(BP.mul(flat(a), BP.W2), 6), n) for g, s, n, a in E6],
           "FQ6_INV": [(g, s, enc(a), tower(BP.inv(flat(a)), 6) if any(a) else [0] * 6, n) for g, s, n, a in E6]}
    assert flat([0, 0, 1, 0]) == BP.W2   # v = w^2
    # a (s0 + s1 v): every Fq6 class beside a random (s0, s1); every Fq2 class as s0 and as s1; the core classes of s0 and s1 in pairs
    m01 = [(g, s, n, a, rand_el(rnd, 2), rand_el(rnd, 2)) for g, s, n, a in E6]
    gen6 = [c[3] for c in E6 if not c[1]]
    for g, s, n, b in E2:
        m01.append(("s0 " + g, s, "s0 " + n, rnd.choice(gen6), b, rand_el(rnd, 2)))
        m01.append(("s1 " + g, s, "s1 " + n, rnd.choice(gen6), rand_el(rnd, 2), b))
    core2 = [c for c in E2 if c[0] in CORE]
    m01 += [("s0 x s1", True, "s0 %s, s1 %s" % (x[2], y[2]), rnd.choice(gen6), x[3], y[3]) for x in core2 for y in core2]
    assert len(m01) == len(E6) + 2 * len(E2) + len(core2) ** 2
    ops["FQ6_MUL_01"] = [(g, s, enc(a + s0 + s1), mul6(a, s0 + s1), n) for g, s, n, a, s0, s1 in m01]
    return ops


def fq12_elements():
    return element_classes(12, random.Random(203))


def fq12_cases():
    rnd = random.Random(204)
    E12, E2, E1 = fq12_elements(), element_classes(2, rnd), element_classes(1, rnd)
    F = {id(c): flat(c[3]) for c in E12}
    inv_in = [c for c in E12 if any(c[3])]   # zero has no inverse: left out by construction
    assert len(inv_in) == len(E12) - 1
    ops = {"FQ12_MUL": [(g, s, enc(a + b), tower(BP.mul(flat(a), flat(b))), n) for g, s, n, a, b in pair_classes(E12, E12, rnd)],
           "FQ12_SQR": [(g, s, enc(a), tower(BP.mul(F[id(c)], F[id(c)])), n) for c in E12 for g, s, n, a in (c,)],
           "FQ12_INV": [(g, s, enc(a), tower(BP.inv(F[id(c)])), n) for c in inv_in for g, s, n, a in (c,)],
           "FQ12_CONJ": [(g, s, enc(a), tower(conj12(F[id(c)])), n) for c in E12 for g, s, n, a in (c,)],
           "FQ12_FROB": [(g, s, enc(a) + word(k), tower(BP.power(F[id(c)], Q ** k)), "%s, k = %d" % (n, k))
                         for c in E12 for g, s, n, a in (c,) for k in (1, 2, 3)]}
    assert len(ops["FQ12_FROB"]) == 3 * len(E12)
    gen12 = [c[3] for c in E12 if not c[1]]
    core12 = [c for c in E12 if c[0] in CORE]
    # f (l0 + l1 w + l3 w^3): every Fq12 class beside a random line; every Fq2 class in each of the three positions; a zero in
    # each position in turn (and in two, and in all) against every core class of f
    ln = [(g, s, n, a, [rand_el(rnd, 2) for _ in range(3)]) for g, s, n, a in E12]
    for pos in range(3):
        for g, s, n, b in E2:
            l = [rand_el(rnd, 2) for _ in range(3)]
            l[pos] = b
            ln.append(("l%d %s" % (pos, g), s, "l%d %s" % (pos, n), rnd.choice(gen12), l))
    zero_masks = (1, 2, 4, 3, 5, 6, 7)
    for m in zero_masks:
        for g, s, n, a in core12:
            ln.append(("zero coefficients", True, "%s, zero mask %d" % (n, m), a, [[0, 0] if m >> p & 1 else rand_el(rnd, 2) for p in range(3)]))
    assert len(ln) == len(E12) + 3 * len(E2) + len(zero_masks) * len(core12)
    ops["FQ12_MUL_LINE"] = [(g, s, enc(a + l[0] + l[1] + l[2]), tower(BP.mul(flat(a), line_flat(*map(tuple, l)))), n) for g, s, n, a, l in ln]
    # the same through a Line and a G1 point: l0 = a yP, l1 = b xP, l3 = c
    at = [(g, s, n, a, l, rand_el(rnd, 2)) for g, s, n, a, l in ln]
    for g, s, n, x in E1:
        at.append(("xP " + g, s, "xP " + n, rnd.choice(gen12), [rand_el(rnd, 2) for _ in range(3)], [x[0], rnd.randrange(1, Q)]))
        at.append(("yP " + g, s, "yP " + n, rnd.choice(gen12), [rand_el(rnd, 2) for _ in range(3)], [rnd.randrange(1, Q), x[0]]))
    assert len(at) == len(ln) + 2 * len(E1)

    def at_want(a, l, p):
        l0, l1 = ((l[0][0] * p[1] % Q, l[0][1] * p[1] % Q), (l[1][0] * p[0] % Q, l[1][1] * p[0] % Q))
        return tower(BP.mul(flat(a), line_flat(l0, l1, tuple(l[2]))))

    ops["FQ12_MUL_LINE_AT"] = [(g, s, enc(a + l[0] + l[1] + l[2] + p), at_want(a, l, p), n) for g, s, n, a, l, p in at]
    return ops


def cyclotomic_elements():
    """the easy part, by the oracle, of every invertible Fq12 class, and 1.  Not -1: the cyclotomic subgroup, where Granger-Scott
    squaring and the hard part's conjugate-for-inverse hold, has the odd order q^4 - q^2 + 1, and (-1)^(q^4 - q^2 + 1) = -1; the
    easy part never yields it (it maps -1 to 1, which FINAL_EASY checks)."""
    E = [c for c in fq12_elements() if any(c[3])]
    out = [("units", True, "one", BP.ONE)]
    out += [("easy part of a " + ("special" if s else "random"), s, "easy part of " + n, easy_of(flat(a))) for g, s, n, a in E]
    assert len(out) == len(fq12_elements())
    return out


def final_cases():
    E = [c for c in fq12_elements() if any(c[3])]
    C = cyclotomic_elements()
    hard = [BP.power(a, HARD_EXP) for *_, a in C]
    for h in hard:   # every input lies in the cyclotomic subgroup: a^(q^4 - q^2 + 1) = (a^HARD_EXP)^R = 1
        assert BP.power(h, R) == BP.ONE
    assert BP.power(BP.f12(Q - 1), HARD_EXP * R) != BP.ONE
    return {"FQ12_CSQ": [(g, s, enc(tower(a)), tower(BP.mul(a, a)), n) for g, s, n, a in C],
            "FINAL_EASY": [(g, s, enc(a), tower(easy_of(flat(a))), n) for g, s, n, a in E],
            "FINAL_HARD": [(g, s, enc(tower(a)), tower(h), n) for (g, s, n, a), h in zip(C, hard)]}


class Step:
    """what a Miller step must give: T afterwards (affine), and the slope and the affine T of before for the line"""

    def __init__(self, t_after, slope, t_before):
        self.t_after, self.slope, self.t_before = t_after, slope, t_before


def steps_cases():
    rnd = random.Random(205)
    G = GF.G2
    logs = [1, 2, R - 1] + [rnd.randrange(3, R - 1) for _ in range(5)]
    qk = [pow(Q, k, R) for k in range(3)]
    pairs = [(a, b) for a in logs for b in logs if a != b and (a + b) % R]
    for k in (1, 2):   # T is neither pi^k(Q) nor its negative
        assert all((a - b * qk[k]) % R and (a + b * qk[k]) % R for a, b in pairs)
    need = sorted(set(logs) | {2 * a % R for a in logs} | {(a + s * b * qk[k]) % R for a, b in pairs for k in range(3) for s in (1, -1)}
                  | {b * qk[k] % R for b in logs for k in (1, 2)} | {-b * qk[2] % R for b in logs})
    pt = dict(zip(need, G.gen_muls(need)))
    assert all(p is not None for p in pt.values())

    def proj(log, scaled):
        z = tuple(rand_el(rnd, 2)) if scaled else (1, 0)
        x, y = pt[log]
        return list(F2.mul(x, z)) + list(F2.mul(y, z)) + list(z)

    def aff(p):
        return list(p[0]) + list(p[1])

    def tangent(log):
        x, y = pt[log]
        return Step(pt[2 * log % R], F2.mul(F2.mul((3, 0), F2.mul(x, x)), F2.inv(F2.add(y, y))), pt[log])

    def chord(a, q, total):
        (x1, y1), (x2, y2) = pt[a], q
        return Step(pt[total % R], F2.mul(F2.sub(y1, y2), F2.inv(F2.sub(x1, x2))), pt[a])

    def cls(log, scaled, *more):
        special = not scaled or log in (1, 2, R - 1) or any(m in (1, 2, R - 1) for m in more)
        return ("Z = 1" if not scaled else "edge logs" if special else "random", special)

    frob = {(b, k): twist_frob(pt[b], k) for b in logs for k in (1, 2)}
    for b in logs:   # pi acts on G2 as multiplication by q
        assert frob[b, 1] == pt[b * qk[1] % R] and frob[b, 2] == pt[b * qk[2] % R]
    ops = {"G2_DBL_STEP": [], "G2_ADD_STEP": [], "MILLER_STEP": [], "G2_FROB1": [], "G2_NEG_FROB2": []}
    for scaled in (False, True):
        for a in logs:
            g, s = cls(a, scaled)
            ops["G2_DBL_STEP"].append((g, s, enc(proj(a, scaled)), tangent(a), "2 T, log %d" % a))
            ops["MILLER_STEP"].append(("kind 0 " + g, s, word(0) + enc(proj(a, scaled) + aff(pt[logs[0]])), tangent(a), "kind 0, log %d" % a))
        for a, b in pairs:
            g, s = cls(a, scaled, b)
            ops["G2_ADD_STEP"].append((g, s, enc(proj(a, scaled) + aff(pt[b])), chord(a, pt[b], a + b), "T + Q, logs %d, %d" % (a, b)))
    for i, (a, b) in enumerate(pairs):
        scaled = i % 3 != 0
        g, s = cls(a, scaled, b)
        ops["MILLER_STEP"].append(("kind 1 " + g, s, word(1) + enc(proj(a, scaled) + aff(pt[b])), chord(a, pt[b], a + b), "kind 1, logs %d, %d" % (a, b)))
        ops["MILLER_STEP"].append(("kind 2 " + g, s, word(2) + enc(proj(a, scaled) + aff(pt[b])), chord(a, frob[b, 1], a + b * qk[1]),
                                   "kind 2, logs %d, %d" % (a, b)))
        nq2 = G.neg_aff(frob[b, 2])
        ops["MILLER_STEP"].append(("kind 3 " + g, s, word(3) + enc(proj(a, scaled) + aff(pt[b])), chord(a, nq2, a - b * qk[2]),
                                   "kind 3, logs %d, %d" % (a, b)))
    for b in logs:
        s = b in (1, 2, R - 1)
        ops["G2_FROB1"].append(("edge logs" if s else "random", s, enc(aff(pt[b])), aff(frob[b, 1]), "pi(Q), log %d" % b))
        ops["G2_NEG_FROB2"].append(("edge logs" if s else "random", s, enc(aff(pt[b])), aff(G.neg_aff(frob[b, 2])), "-pi^2(Q), log %d" % b))
    n, p = len(logs), len(pairs)
    assert p == n * (n - 1) - 2   # (1, R - 1) and (R - 1, 1) sum to O
    assert [len(ops[o]) for o in ("G2_DBL_STEP", "G2_ADD_STEP", "MILLER_STEP", "G2_FROB1", "G2_NEG_FROB2")] == [2 * n, 2 * p, 2 * n + 3 * p, n, n]
    return ops


_BUILDERS = {"fq2": fq2_cases, "fq6": fq6_cases, "fq12": fq12_cases, "final": final_cases, "steps": steps_cases}


# -- arrangement -------------------------------------------------------------------------------------------------------------------
def arrange(cases, rnd):
    """the cases in lane order: first waves of one group each (its cases repeated to fill the wave), then waves with a special
    case at lane 0, lane 63 and every even lane between generic ones"""
    by_group = {}
    for c in cases:
        by_group.setdefault(c[0], []).append(c)
    out = []
    for members in by_group.values():
        n = -(-len(members) // 64) * 64
        out += [members[i % len(members)] for i in range(n)]
    special = [c for c in cases if c[1]]
    generic = [c for c in cases if not c[1]]
    assert special and generic
    rnd.shuffle(special)
    waves = max(3, -(-len(special) // 33))
    s = g = 0
    for _ in range(waves):
        for lane in range(64):
            if lane % 2 == 0 or lane == 63:
                out.append(special[s % len(special)])
                s += 1
            else:
                out.append(generic[g % len(generic)])
                g += 1
    assert s >= len(special) and len(out) % 64 == 0 and len(out) // 64 >= 5   # several workgroups
    return out


@functools.lru_cache(maxsize=None)
def family(name):
    """-> [(op name, cases in lane order)]: built once, shared by the CPU and the GPU test"""
    ops = _BUILDERS[name]()
    assert list(ops) != [] and set(ops) == set(FAMILIES[name])
    rnd = random.Random(name)
    return [(op, arrange(ops[op], rnd)) for op in FAMILIES[name]]


def build_device_harness(out_dir, hipcc="hipcc"):
    """compiles tests/native/fq12_tower.hip for gfx950, one program per family side by side -> {family: executable}"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exes = {name: os.path.join(str(out_dir), "fq12_tower_" + name) for name in FAMILIES}
    procs = [(name, subprocess.Popen([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-DTOWER_FAMILY=%d" % (i + 1),
                                      "-I" + os.path.join(root, "circom-witnesscalc_amd", "r1cs"), os.path.join(root, "tests", "native", "fq12_tower.hip"),
                                      "-o", exes[name]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
             for i, name in enumerate(FAMILIES)]
    for name, p in procs:
        out, _ = p.communicate(timeout=1800)
        assert p.returncode == 0, "family %s: hipcc exit status %d\n%s" % (name, p.returncode, out[-4000:])
    return exes


def write_sections(path, sections):
    with open(path, "wb") as f:
        for op, cases in sections:
            rec = b"".join(c[2] for c in cases)
            assert len(rec) == 4 * IN_WORDS[op] * len(cases) and len(cases) % 64 == 0
            f.write(np.array([OP[op], len(cases), IN_WORDS[op], OUT_WORDS[op], 0], dtype="<u4").tobytes())
            f.write(rec)


# -- comparison --------------------------------------------------------------------------------------------------------------------
def check_step(words, want, what):
    v = dec(words, what)
    X, Y, Z, a, b, c = (tuple(v[2 * i:2 * i + 2]) for i in range(6))
    assert Z != (0, 0), what + ": Z = 0"
    zi = F2.inv(Z)
    assert (F2.mul(X, zi), F2.mul(Y, zi)) == want.t_after, what + ": T after the step"
    assert a != (0, 0), what + ": the line's a is zero"
    xt, yt = want.t_before
    assert b == F2.mul(F2.neg(want.slope), a), what + ": b is not -s a"
    assert c == F2.mul(F2.sub(F2.mul(want.slope, xt), yt), a), what + ": c is not (s x_T - y_T) a"


def check_outputs(path, sections):
    """the program's output file against the expected values: exact equality of canonical values, every coefficient below q,
    the guard records after each section untouched"""
    raw = np.fromfile(path, dtype="<u4")
    pos = 0
    for op, cases in sections:
        ow, n = OUT_WORDS[op], len(cases)
        got = raw[pos:pos + n * ow].reshape(n, ow)
        guard = raw[pos + n * ow:pos + (n + GUARD) * ow]
        pos += (n + GUARD) * ow
        assert guard.size == GUARD * ow and (guard == 0xa5a5a5a5).all(), "%s: words past the last record were written" % op
        seen = {}
        for lane, (group, _, rec, want, name) in enumerate(cases):
            what = "%s %s (%s), record %d (lane %d)" % (op, name, group, lane, lane % 64)
            key = (rec, got[lane].tobytes())
            if key in seen:   # the same record with the same words as a lane already checked
                continue
            if isinstance(want, Step):
                check_step(got[lane], want, what)
            else:
                assert dec(got[lane], what) == list(want), what
            seen[key] = True
    assert pos == raw.size
