"""A plain-Python model of the compressed point form (include/graph_witness_groth16_compressed.h: arkworks 0.4
CanonicalSerialize, Compress::Yes, restated), on integers only, and the case lists of the point-codec tests
(tests/test_point_codec_host.py on the CPU, tests/test_gpu_point_codec.py, tests/test_gpu_point_codec_api.py and
tests/test_gpu_groth16_compressed.py on an MI355X).

Roots in Fq are pow(a, (q + 1) / 4, q).  Roots in Fq2 come by another route than the header's (which goes through the norm): the
"complex method" for q = 3 mod 4 of Adj and Rodriguez-Henriquez, a1 = a^((q - 3) / 4), alpha = a1^2 a, no root iff
alpha^(q + 1) = -1, x0 = a1 a, the root u x0 when alpha = -1, else (1 + alpha)^((q - 1) / 2) x0.  kernel_branch() follows the
header's route far enough to say which of its two cases an input takes, so that the lists hold both.

The records of tests/native/point_codec.hip (layouts: tests/native/point_codec_ops.hpp) are sections in the format of
tests/native/fq12_tower.hip; a case is (group, special, record bytes, check, name) as in tests/fq12_tower_cases.py, whose lane
arrangement is used: `check(words)` asserts on the result words of the record."""
import functools
import os
import random
import re
import subprocess

import numpy as np

from tests import fq12_tower_cases as TC
from tests import groth16_fixtures as GF

Q, R, MONT = GF.Q, GF.R, GF.MONT
MONT_INV = pow(MONT, -1, Q)
F2 = GF.Fq2
HALF = (Q - 1) // 2
SQRT_EXP = (Q + 1) // 4
FLAG_LARGER, FLAG_INFINITY = 0x80, 0x40
VALID, POINT = 0, 2
GUARD = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "circom-witnesscalc_amd", "r1cs", "point_codec_gfx950.hpp")
assert Q % 4 == 3 and Q < 1 << 254


# -- square roots ----------------------------------------------------------------------------------------------------------------
def fq_sqrt(a):
    """the root pow(a, (q + 1) / 4), or None when a is no square"""
    r = pow(a, SQRT_EXP, Q)
    return r if r * r % Q == a % Q else None


def fq2_pow(a, e):
    acc = (1, 0)
    for bit in bin(e)[2:]:
        acc = F2.mul(acc, acc)
        if bit == "1":
            acc = F2.mul(acc, a)
    return acc


def fq2_sqrt(a):
    """a root of a in Fq2 or None, by the complex method (not the header's route)"""
    a = (a[0] % Q, a[1] % Q)
    if a == (0, 0):
        return (0, 0)
    a1 = fq2_pow(a, (Q - 3) // 4)
    alpha = F2.mul(F2.mul(a1, a1), a)
    a0 = F2.mul((alpha[0], -alpha[1] % Q), alpha)   # alpha^q alpha
    if a0 == (Q - 1, 0):
        return None
    x0 = F2.mul(a1, a)
    if alpha == (Q - 1, 0):
        x = F2.mul((0, 1), x0)
    else:
        x = F2.mul(fq2_pow(((1 + alpha[0]) % Q, alpha[1]), (Q - 1) // 2), x0)
    assert F2.mul(x, x) == a
    return x


def kernel_branch(a):
    """which case of the header's fq2_sqrt an input takes: "none" (the norm is no square), "zero", "plus" (c^2 = t) or "minus" """
    n = (a[0] * a[0] + a[1] * a[1]) % Q
    s = fq_sqrt(n)
    if s is None:
        return "none"
    t = (a[0] + s) % Q or (a[0] - s) % Q
    t = t * pow(2, -1, Q) % Q
    if t == 0:
        return "zero"
    c = pow(t, SQRT_EXP, Q)
    return "plus" if c * c % Q == t else "minus"


# -- the format ------------------------------------------------------------------------------------------------------------------
def fq_is_larger(y):
    return y > Q - y if y else False


def fq2_is_larger(y):
    return fq_is_larger(y[1]) if y[1] else fq_is_larger(y[0])


def _le(v):
    return int(v).to_bytes(32, "little")


def _flag(b, f):
    b = bytearray(b)
    b[-1] |= f
    return bytes(b)


def g1_compress(p):
    """affine (x, y) or None (infinity) -> 32 bytes"""
    if p is None:
        return _flag(bytes(32), FLAG_INFINITY)
    return _flag(_le(p[0]), FLAG_LARGER if fq_is_larger(p[1]) else 0)


def g2_compress(p):
    """affine ((x0, x1), (y0, y1)) or None -> 64 bytes"""
    if p is None:
        return _flag(bytes(64), FLAG_INFINITY)
    return _flag(_le(p[0][0]) + _le(p[0][1]), FLAG_LARGER if fq2_is_larger(p[1]) else 0)


def _decode(b, width):
    """-> "inf", None (refused) or (coefficients of x, larger?)"""
    flags = b[-1] & 0xc0
    body = bytearray(b)
    body[-1] &= 0x3f
    if flags == 0xc0:
        return None
    if flags == FLAG_INFINITY:
        return "inf" if not any(body) else None
    x = [int.from_bytes(body[32 * i:32 * i + 32], "little") for i in range(width)]
    if any(c >= Q for c in x):
        return None
    return x, flags == FLAG_LARGER


def g1_decompress(b):
    """32 bytes -> (status, point): (VALID, (x, y)), (VALID, None) for infinity, (POINT, None) for a refused encoding"""
    d = _decode(bytes(b), 1)
    if d is None or d == "inf":
        return (POINT if d is None else VALID), None
    (x,), larger = d
    y = fq_sqrt((x * x * x + 3) % Q)
    if y is None or (y == 0 and larger):
        return POINT, None
    if y and fq_is_larger(y) != larger:
        y = Q - y
    return VALID, (x, y)


def g2_decompress(b):
    d = _decode(bytes(b), 2)
    if d is None or d == "inf":
        return (POINT if d is None else VALID), None
    x, larger = tuple(d[0]), d[1]
    y = fq2_sqrt(F2.add(F2.mul(F2.mul(x, x), x), GF.B2))
    if y is None or (y == (0, 0) and larger):
        return POINT, None
    if y != (0, 0) and fq2_is_larger(y) != larger:
        y = F2.neg(y)
    return VALID, (x, y)


def g1_point(b):
    """64 canonical bytes -> affine point or None"""
    return None if not any(b) else (int.from_bytes(b[:32], "little"), int.from_bytes(b[32:64], "little"))


def g2_point(b):
    if not any(b):
        return None
    v = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(4)]
    return ((v[0], v[1]), (v[2], v[3]))


def g1_bytes(p, mont=False):
    m = MONT if mont else 1
    return bytes(64) if p is None else _le(p[0] * m % Q) + _le(p[1] * m % Q)


def g2_bytes(p, mont=False):
    m = MONT if mont else 1
    return bytes(128) if p is None else b"".join(_le(v * m % Q) for v in (p[0][0], p[0][1], p[1][0], p[1][1]))


def proof_compress(proof):
    """256 proof bytes (A, B, C canonical) -> 128"""
    p = bytes(proof)
    return g1_compress(g1_point(p[:64])) + g2_compress(g2_point(p[64:192])) + g1_compress(g1_point(p[192:256]))


def key_compress(points, n_public):
    """the verifying key's points (alpha1, beta2, gamma2, delta2, IC: Groth16VerifyingKey.points()) -> its compressed bytes"""
    p = bytes(points)
    assert len(p) == 448 + 64 * (n_public + 1)
    out = g1_compress(g1_point(p[:64])) + b"".join(g2_compress(g2_point(p[64 + 128 * k:192 + 128 * k])) for k in range(3))
    out += (n_public + 1).to_bytes(8, "little")
    out += b"".join(g1_compress(g1_point(p[448 + 64 * i:512 + 64 * i])) for i in range(n_public + 1))
    assert len(out) == 232 + 32 * (n_public + 1)
    return out


# -- anchors of the restatement, and the header's constants ------------------------------------------------------------------------
assert g1_compress((1, 2)) == bytes([1]) + bytes(31)
assert g1_compress((1, Q - 2)) == bytes([1]) + bytes(30) + bytes([0x80])
assert g1_compress(None) == bytes(31) + bytes([0x40]) and g2_compress(None) == bytes(63) + bytes([0x40])
assert GF.G2_GEN[1][1] < HALF and g2_compress(GF.G2_GEN) == _le(GF.G2_GEN[0][0]) + _le(GF.G2_GEN[0][1])
assert g1_decompress(g1_compress((1, 2))) == (VALID, (1, 2)) and g1_decompress(g1_compress((1, Q - 2))) == (VALID, (1, Q - 2))
assert g2_decompress(g2_compress(GF.G2_GEN)) == (VALID, GF.G2_GEN)
assert g2_decompress(g2_compress(GF.G2.neg_aff(GF.G2_GEN))) == (VALID, GF.G2.neg_aff(GF.G2_GEN))


def header_constants():
    """{name: integer} of the limb lists in the header: the root's exponent, (q - 1) / 2 and 1/2 in Montgomery form"""
    txt = open(HEADER).read()

    def limbs(pattern):
        m = re.search(pattern + r"[^{]*\{+([^}]*)\}", txt)
        w = [int(x.rstrip("u"), 16) for x in re.findall(r"0x[0-9a-fA-F]+u?", m.group(1))]
        assert len(w) == 8
        return sum(v << (32 * i) for i, v in enumerate(w))

    return {"sqrt_exp": limbs(r"#define CWC_QP1D4_LIMBS"), "half_q": limbs(r"Fq fq_half_q\(\)"), "inv2": limbs(r"Fq fq_inv2\(\)")}


def check_header_constants():
    c = header_constants()
    assert c["sqrt_exp"] == SQRT_EXP and 4 * c["sqrt_exp"] == Q + 1
    assert c["half_q"] == HALF
    assert c["inv2"] == pow(2, -1, Q) * MONT % Q
    assert SQRT_EXP.bit_length() == 252   # the loop of fq_pow_qp1d4 starts at bit 251


# -- points for the API tests ----------------------------------------------------------------------------------------------------
def no_root_x(group, rnd):
    """an x below q (G2: a pair) for which x^3 + b has no root, found by stepping from a seeded start"""
    if group == 1:
        x = rnd.randrange(Q)
        while fq_sqrt((x * x * x + 3) % Q) is not None:
            x = (x + 1) % Q
        return x
    x = (rnd.randrange(Q), rnd.randrange(Q))
    while fq2_sqrt(F2.add(F2.mul(F2.mul(x, x), x), GF.B2)) is not None:
        x = ((x[0] + 1) % Q, x[1])
    return x


@functools.lru_cache(maxsize=None)
def sample_points(group, n, seed=77):
    """n points of the group: a seeded multiple of the generator and its negative by turns, infinity at every 7th place from 3"""
    rnd = random.Random(seed * 10 + group)
    C = GF.G1 if group == 1 else GF.G2
    base = C.gen_muls([rnd.randrange(1, R) for _ in range((n + 1) // 2)])
    out = []
    for i in range(n):
        p = base[i // 2]
        out.append(None if i % 7 == 3 else C.neg_aff(p) if i % 2 else p)
    return tuple(out)


def refused_encodings(group, rnd):
    """[(name, bytes)] of encodings that decoding must refuse"""
    w = 32 * group
    good = bytearray((g1_compress if group == 1 else g2_compress)(sample_points(group, 1)[0]))
    good[-1] &= 0x3f
    out = [("both flags", _flag(good, 0xc0)), ("both flags, zero x", _flag(bytes(w), 0xc0)),
           ("infinity flag with bit 0", _flag(bytes([1]) + bytes(w - 1), FLAG_INFINITY)),
           ("infinity flag with the top bit of x", _flag(bytes(w - 1) + bytes([0x20]), FLAG_INFINITY))]
    for name, v in (("x = q", Q), ("x = 2^254 - 1", (1 << 254) - 1)):
        if group == 1:
            out.append((name, _le(v)))
            out.append((name + ", larger", _flag(_le(v), FLAG_LARGER)))
        else:
            out.append(("c0: " + name, _le(v) + bytes(good[32:])))
            out.append(("c1: " + name, bytes(good[:32]) + _le(v)))
    if group == 2:
        out.append(("infinity flag with a bit of c0", _flag(bytes(31) + bytes([1]) + bytes(32), FLAG_INFINITY)))
        out.append(("a flag bit in c0", bytes(good[:31]) + bytes([good[31] | 0x80]) + bytes(good[32:])))
    for k in range(3):
        x = no_root_x(group, rnd)
        b = _le(x) if group == 1 else _le(x[0]) + _le(x[1])
        out.append(("no root %d" % k, _flag(b, FLAG_LARGER if k == 1 else 0)))
    for name, b in out:
        assert len(b) == w and (g1_decompress if group == 1 else g2_decompress)(b) == (POINT, None), name
    return out


# -- the records of tests/native/point_codec.hip -------------------------------------------------------------------------------------
_NAMES = "FQ_SQRT FQ2_SQRT FQ_IS_LARGER FQ2_IS_LARGER G1_ENCODE G2_ENCODE G1_DECODE G2_DECODE".split()
OP = {n: i + 1 for i, n in enumerate(_NAMES)}
IN_WORDS = dict(FQ_SQRT=8, FQ2_SQRT=16, FQ_IS_LARGER=8, FQ2_IS_LARGER=16, G1_ENCODE=17, G2_ENCODE=33, G1_DECODE=9, G2_DECODE=17)
OUT_WORDS = dict(FQ_SQRT=9, FQ2_SQRT=17, FQ_IS_LARGER=1, FQ2_IS_LARGER=1, G1_ENCODE=8, G2_ENCODE=16, G1_DECODE=17, G2_DECODE=33)
FAMILIES = {"roots": _NAMES[:2], "order": _NAMES[2:4], "codec": _NAMES[4:]}


def enc(vals):
    return b"".join(_le(v * MONT % Q) for v in vals)


def raw(vals):
    return b"".join(_le(v) for v in vals)


def _ints(words):
    b = np.ascontiguousarray(words, dtype="<u4").tobytes()
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(b) // 32)]


def _want_words(b):
    return lambda w, what: _assert_eq(np.ascontiguousarray(w, dtype="<u4").tobytes(), b, what)


def _assert_eq(got, want, what):
    assert got == want, "%s: %s, expected %s" % (what, got.hex(), want.hex())


def _check_fq_sqrt(a):
    def check(w, what):
        (r,) = _ints(w[:8])
        assert r < Q, what + ": the root is not reduced"
        assert r * MONT_INV % Q == pow(a, SQRT_EXP, Q), what + ": not a^((q + 1) / 4)"
        assert int(w[8]) == (1 if fq_sqrt(a) is not None else 0), what + ": the verdict"
        if int(w[8]):
            assert (r * MONT_INV) ** 2 % Q == a, what + ": root^2 != a"
    return check


def _check_fq2_sqrt(a):
    want = fq2_sqrt(a)

    def check(w, what):
        r = _ints(w[:16])
        assert all(c < Q for c in r), what + ": the root is not reduced"
        assert int(w[16]) == (0 if want is None else 1), what + ": the verdict"
        if want is not None:
            root = (r[0] * MONT_INV % Q, r[1] * MONT_INV % Q)
            assert F2.mul(root, root) == a, what + ": root^2 != a"
            assert root in (want, F2.neg(want)), what + ": not one of the two roots"
    return check


def roots_cases():
    rnd = random.Random(301)
    f = [("edges", True, "0", 0), ("edges", True, "1", 1), ("edges", True, "4", 4), ("edges", True, "q - 1", Q - 1),
         ("edges", True, "(q - 1) / 2", HALF), ("edges", True, "(q + 1) / 2", HALF + 1)]
    assert fq_sqrt(Q - 1) is None and fq_sqrt(4) in (2, Q - 2)
    res, non = [], []
    while len(res) < 32 or len(non) < 32:
        a = rnd.randrange(1, Q)
        (res if fq_sqrt(a) is not None else non).append(a)
    f += [("residues", False, "residue", a) for a in res[:32]] + [("non-residues", False, "non-residue", a) for a in non[:32]]
    ops = {"FQ_SQRT": [(g, s, enc([a]), _check_fq_sqrt(a), n) for g, s, n, a in f]}
    r0, n0 = res[0], non[0]
    g = [("edges", True, "(0, 0)", (0, 0)), ("edges", True, "(1, 0)", (1, 0)), ("edges", True, "(-1, 0)", (Q - 1, 0)),
         ("edges", True, "(residue, 0)", (r0, 0)), ("edges", True, "(non-residue, 0)", (n0, 0)), ("edges", True, "(0, a1)", (0, rnd.randrange(1, Q))),
         ("edges", True, "(0, 1)", (0, 1)), ("edges", True, "(0, non-residue)", (0, n0))]
    assert fq2_sqrt((n0, 0))[0] == 0 and fq2_sqrt((r0, 0))[1] == 0   # a pure-imaginary root, a real root
    by = {"none": [], "plus": [], "minus": []}
    while min(len(v) for v in by.values()) < 8:
        a = (rnd.randrange(Q), rnd.randrange(1, Q))
        if rnd.random() < 0.7:
            a = F2.mul(a, a)
        by[kernel_branch(a)].append(a)
    for k, v in by.items():
        assert all((fq2_sqrt(a) is None) == (k == "none") for a in v)
        g += [("branch " + k, True, "branch " + k, a) for a in v[:8]]
    for _ in range(64):
        x = (rnd.randrange(Q), rnd.randrange(Q))
        g.append(("squares", False, "seeded square", F2.mul(x, x)))
    assert {kernel_branch(a) for *_, a in g} == {"none", "zero", "plus", "minus"}
    ops["FQ2_SQRT"] = [(gr, s, enc(a), _check_fq2_sqrt(a), n) for gr, s, n, a in g]
    return ops


def crossing_values(rnd, n):
    """values whose canonical and Montgomery forms lie on opposite sides of (q - 1) / 2"""
    out = []
    while len(out) < n:
        v = rnd.randrange(1, Q)
        if (v > HALF) != (v * MONT % Q > HALF):
            out.append(v)
    return out


def order_cases():
    rnd = random.Random(302)
    one = lambda flag: _want_words((1 if flag else 0).to_bytes(4, "little"))  # noqa: E731
    f = [("edges", True, n, v) for n, v in (("0", 0), ("1", 1), ("q - 1", Q - 1), ("(q - 1) / 2", HALF), ("(q + 1) / 2", HALF + 1))]
    cross = crossing_values(rnd, 12)
    assert len(cross) >= 8
    f += [("crossing", True, "canonical and Montgomery on opposite sides", v) for v in cross]
    f += [("random", False, "random", rnd.randrange(Q)) for _ in range(16)]
    assert not fq_is_larger(HALF) and fq_is_larger(HALF + 1) and fq_is_larger(Q - 1) and not fq_is_larger(1) and not fq_is_larger(0)
    ops = {"FQ_IS_LARGER": [(g, s, raw([v]), one(fq_is_larger(v)), n) for g, s, n, v in f]}
    c0 = rnd.randrange(1, Q)
    g = [("c1 = 0", True, "c1 = 0, c0 = %s" % n, (v, 0)) for n, v in (("0", 0), ("1", 1), ("q - 1", Q - 1), ("(q - 1) / 2", HALF), ("(q + 1) / 2", HALF + 1))]
    g += [("c1 at the middle", True, "c1 = (q - 1) / 2", (Q - 1, HALF)), ("c1 at the middle", True, "c1 = (q + 1) / 2", (1, HALF + 1)),
          ("c1 at the middle", True, "c1 = (q - 1) / 2, c0 = 0", (0, HALF)), ("c1 at the middle", True, "c1 = (q + 1) / 2, c0 = 0", (0, HALF + 1))]
    for c1 in (rnd.randrange(1, HALF), rnd.randrange(HALF + 1, Q)):
        g += [("equal c1", True, "equal c1, c0 small", (1, c1)), ("equal c1", True, "equal c1, c0 large", (Q - 1, c1)),
              ("equal c1", True, "equal c1, c0 random", (c0, c1))]
    g += [("crossing", True, "c1 crossing", (rnd.randrange(Q), v)) for v in cross]
    g += [("crossing", True, "c0 crossing, c1 = 0", (v, 0)) for v in cross]
    g += [("random", False, "random", (rnd.randrange(Q), rnd.randrange(Q))) for _ in range(16)]
    ops["FQ2_IS_LARGER"] = [(gr, s, raw(a), one(fq2_is_larger(a)), n) for gr, s, n, a in g]
    return ops


def codec_cases():
    rnd = random.Random(303)
    ops = {n: [] for n in FAMILIES["codec"]}
    for group, pb, comp, dec, name in ((1, g1_bytes, g1_compress, g1_decompress, "G1"), (2, g2_bytes, g2_compress, g2_decompress, "G2")):
        pts = sample_points(group, 24)
        ybig = [p for p in pts if p is not None and (fq_is_larger(p[1]) if group == 1 else fq2_is_larger(p[1]))]
        assert ybig and len(ybig) < len([p for p in pts if p is not None])
        for form in (0, 1):
            fw = form.to_bytes(4, "little")
            for i, p in enumerate(pts):
                special = p is None or i < 4
                grp = "infinity" if p is None else "form %d" % form
                c = comp(p)
                ops[name + "_ENCODE"].append((grp, special, fw + pb(p, form == 1), _want_words(c), "%s point %d, form %d" % (name, i, form)))
                ops[name + "_DECODE"].append((grp, special, fw + c, _want_words(pb(p, form == 1) + bytes(4)), "%s point %d, form %d" % (name, i, form)))
            for n, b in refused_encodings(group, rnd):
                ops[name + "_DECODE"].append(("refused", True, fw + b, _want_words(bytes(64 * group) + POINT.to_bytes(4, "little")),
                                              "%s %s, form %d" % (name, n, form)))
    return ops


_BUILDERS = {"roots": roots_cases, "order": order_cases, "codec": codec_cases}


@functools.lru_cache(maxsize=None)
def family(name):
    """-> [(op name, cases in lane order)], built once and shared by the CPU and the GPU test"""
    ops = _BUILDERS[name]()
    assert set(ops) == set(FAMILIES[name])
    rnd = random.Random("point codec " + name)
    return [(op, TC.arrange(ops[op], rnd)) for op in FAMILIES[name]]


def write_sections(path, sections):
    with open(path, "wb") as f:
        for op, cases in sections:
            rec = b"".join(c[2] for c in cases)
            assert len(rec) == 4 * IN_WORDS[op] * len(cases) and len(cases) % 64 == 0
            f.write(np.array([OP[op], len(cases), IN_WORDS[op], OUT_WORDS[op], 0], dtype="<u4").tobytes())
            f.write(rec)


def check_outputs(path, sections):
    """the program's output file: every record's check, and the guard records after each section untouched"""
    out = np.fromfile(path, dtype="<u4")
    pos = 0
    for op, cases in sections:
        ow, n = OUT_WORDS[op], len(cases)
        got = out[pos:pos + n * ow].reshape(n, ow)
        guard = out[pos + n * ow:pos + (n + GUARD) * ow]
        pos += (n + GUARD) * ow
        assert guard.size == GUARD * ow and (guard == 0xa5a5a5a5).all(), "%s: words past the last record were written" % op
        seen = set()
        for lane, (group, _, rec, check, name) in enumerate(cases):
            key = (rec, got[lane].tobytes())
            if key in seen:
                continue
            check(got[lane], "%s %s (%s), record %d (lane %d)" % (op, name, group, lane, lane % 64))
            seen.add(key)
    assert pos == out.size


def build_device_harness(out_dir, hipcc="hipcc"):
    """compiles tests/native/point_codec.hip for gfx950 -> the executable"""
    exe = os.path.join(str(out_dir), "point_codec")
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "circom-witnesscalc_amd", "r1cs"),
                        os.path.join(ROOT, "tests", "native", "point_codec.hip"), "-o", exe], capture_output=True, text=True, timeout=1800)
    assert p.returncode == 0, "hipcc exit status %d\n%s" % (p.returncode, (p.stdout + p.stderr)[-4000:])
    return exe
