"""The G1 / G2 group law of r1cs/fq_gfx950.hpp on a real MI355X at its special cases, alone and diverging inside one wave.

tests/native/bn254_group.hip (compiled here) runs xyzz_add, xyzz_add_affine, xyzz_dbl, xyzz_neg, xyzz_to_affine, xyzz_mul and
xyzz_mul_short for both groups in full 64-lane waves over several workgroups, one operand record per lane, and returns raw XYZZ
limbs.  The reference is groth16_fixtures.Curve with Python integers: operands are multiples a G of the generators, each given
as (l^2 x, l^3 y, l^2, l^3) under a random scaling l and with l = 1, and the expected point is the multiple with the expected
log.  A result must satisfy ZZ^3 == ZZZ^2, be the point at infinity exactly when ZZ == 0, and have X / ZZ, Y / ZZZ equal to the
reference; the affine form the device derives from a result (xyzz_to_affine, (0, 0) for infinity) is compared directly.

Every case runs twice: in waves whose 64 lanes all take the same branch, and in waves where special and generic lanes are
interleaved (special at lane 0, lane 63 and every even lane), where an early return of one lane meets the others' work.
One process under one time limit per family; after a process that did not exit with status 0 no further family is started."""
import os
import random
import subprocess

import numpy as np
import pytest

from tests import groth16_fixtures as GF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, Q, MONT = GF.R, GF.Q, GF.MONT
MONT_INV = pow(MONT, -1, Q)
OP = dict(ADD=1, ADD_AFFINE=2, DBL=3, NEG=4, TO_AFFINE=5, MUL=6, MUL_SHORT=7)
N_LOGS = 12
_state = {"failed": None}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bn254_group") / "bn254_group"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "circom-witnesscalc_amd", "r1cs"),
                    os.path.join(ROOT, "tests", "native", "bn254_group.hip"), "-o", str(exe)], check=True, timeout=1800)
    return str(exe)


def run_family(exe, tmp_path, name, sections, timeout=240):
    """sections: [(op, records u32 [n, iw], out_words, group)] -> [u32 [n, ow]]"""
    if _state["failed"]:
        pytest.fail("not started: the harness process of family %r did not exit cleanly" % _state["failed"])
    fin, fout = tmp_path / (name + ".in"), tmp_path / (name + ".out")
    with open(fin, "wb") as f:
        for op, rec, ow, group in sections:
            rec = np.ascontiguousarray(rec, dtype="<u4")
            assert rec.shape[0] % 64 == 0
            f.write(np.array([op, rec.shape[0], rec.shape[1], ow, group], dtype="<u4").tobytes())
            f.write(rec.tobytes())
    p = subprocess.run(["timeout", "-k", "10", str(timeout), exe, str(fin), str(fout)], capture_output=True, text=True)
    if p.returncode != 0:
        _state["failed"] = name
        pytest.fail("harness family %r: exit status %d\n%s\n%s" % (name, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
    raw = np.fromfile(fout, dtype="<u4")
    out, pos = [], 0
    for op, rec, ow, group in sections:
        n = rec.shape[0]
        out.append(raw[pos:pos + n * ow].reshape(n, ow))
        pos += n * ow
    assert pos == raw.size
    return out


class Group:
    """one of the two groups: encoding of coordinates as Montgomery limbs, scalings, and multiples of the generator by log"""

    def __init__(self, curve, group, seed):
        self.curve, self.f, self.id = curve, curve.f, group
        self.w = 8 * group                     # words per coordinate
        self.rnd = random.Random(seed)
        self.logs = [1, 2, R - 1] + [self.rnd.randrange(1, R) for _ in range(N_LOGS - 3)]
        self.known = {0: None}

    def need(self, logs):
        todo = sorted({k % R for k in logs} - set(self.known))
        self.known.update(zip(todo, self.curve.gen_muls(todo)))

    def point(self, log):
        return self.known[log % R]

    def el(self, x):
        """field element -> bytes of its Montgomery limbs"""
        return b"".join((c * MONT % Q).to_bytes(32, "little") for c in ((x,) if self.id == 1 else x))

    def un(self, words):
        """u32 words of one coordinate -> field element"""
        raw = words.astype("<u4").tobytes()
        cs = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(self.id)]
        assert all(c < Q for c in cs), "a coordinate is not reduced"
        cs = [c * MONT_INV % Q for c in cs]
        return cs[0] if self.id == 1 else tuple(cs)

    def rand_el(self):
        while True:
            x = self.rnd.randrange(1, Q) if self.id == 1 else (self.rnd.randrange(Q), self.rnd.randrange(Q))
            if x != self.f.zero:
                return x

    def xyzz(self, log, scaled=True, junk=False):
        """bytes of log G as XYZZ: scaled by a random l or with l = 1; infinity as zeros, or with junk in X and Y"""
        f, p = self.f, self.point(log)
        if p is None:
            x, y = (self.rand_el(), self.rand_el()) if junk else (f.zero, f.zero)
            return self.el(x) + self.el(y) + self.el(f.zero) + self.el(f.zero)
        lam = self.rand_el() if scaled else f.one
        l2 = f.mul(lam, lam)
        l3 = f.mul(l2, lam)
        return self.el(f.mul(p[0], l2)) + self.el(f.mul(p[1], l3)) + self.el(l2) + self.el(l3)

    def affine(self, log):
        p = self.point(log)
        assert p is not None
        return self.el(p[0]) + self.el(p[1])

    def check_xyzz(self, words, log, what):
        f, w = self.f, self.w
        X, Y, ZZ, ZZZ = (self.un(words[i * w:(i + 1) * w]) for i in range(4))
        assert f.mul(f.mul(ZZ, ZZ), ZZ) == f.mul(ZZZ, ZZZ), what + ": ZZ^3 != ZZZ^2"
        want = self.point(log)
        if want is None:
            assert ZZ == f.zero, what + ": expected the point at infinity"
            return
        assert ZZ != f.zero, what + ": infinity, expected a point"
        assert (f.mul(X, f.inv(ZZ)), f.mul(Y, f.inv(ZZZ))) == want, what

    def check_affine(self, words, log, what):
        w = self.w
        got = (self.un(words[:w]), self.un(words[w:2 * w]))
        want = self.point(log)
        assert got == ((self.f.zero, self.f.zero) if want is None else want), what


GROUPS = {"G1": lambda: Group(GF.G1, 1, 11), "G2": lambda: Group(GF.G2, 2, 12)}


def arrange(cases, rnd):
    """cases: [(class, special, record bytes, expected)] -> the list in lane order: first waves of one class each (its cases
    repeated to fill the wave), then waves with a special case at lane 0, lane 63 and every even lane between generic ones"""
    by_class = {}
    for c in cases:
        by_class.setdefault(c[0], []).append(c)
    out = []
    for members in by_class.values():
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
    assert s >= len(special) and len(out) % 64 == 0 and len(out) // 64 >= 5  # (several workgroups of four waves)
    return out


def records(cases):
    n = len(cases)
    return np.frombuffer(b"".join(c[2] for c in cases), dtype="<u4").reshape(n, -1)


def addition_cases(G):
    """-> {op: cases} for add, add_affine, dbl, neg, to_affine; expected: the log of the result"""
    rnd, L = G.rnd, G.logs
    pairs = [(a, b) for a in L for b in L if (a + b) % R and a != b]
    rnd.shuffle(pairs)
    G.need(L + [-a for a in L] + [a + b for a, b in pairs[:48]] + [2 * a for a in L])
    forms = [(True, True), (True, False), (False, True), (False, False)]  # which operand is scaled
    add, aff, dbl, neg, toa = [], [], [], [], []
    for i, (a, b) in enumerate(pairs[:48]):
        sa, sb = forms[i % 4]
        add.append(("generic", False, G.xyzz(a, sa) + G.xyzz(b, sb), a + b))
        aff.append(("generic", False, G.xyzz(a, sa) + G.affine(b), a + b))
    for i, a in enumerate(L):
        for sa, sb in forms:
            add.append(("P + P", True, G.xyzz(a, sa) + G.xyzz(a, sb), 2 * a))
            add.append(("P + (-P)", True, G.xyzz(a, sa) + G.xyzz(-a, sb), 0))
        for junk in (False, True):
            add.append(("O + P", True, G.xyzz(0, junk=junk) + G.xyzz(a, i % 2 == 0), a))
            add.append(("P + O", True, G.xyzz(a, i % 2 == 1) + G.xyzz(0, junk=junk), a))
            aff.append(("O + P", True, G.xyzz(0, junk=junk) + G.affine(a), a))
        add.append(("O + O", True, G.xyzz(0, junk=i % 2 == 0) + G.xyzz(0, junk=i % 3 == 0), 0))
        for sa in (True, False):
            aff.append(("P + P", True, G.xyzz(a, sa) + G.affine(a), 2 * a))
            aff.append(("P + (-P)", True, G.xyzz(a, sa) + G.affine(-a), 0))
            dbl.append(("generic", False, G.xyzz(a, sa), 2 * a))
            neg.append(("generic", False, G.xyzz(a, sa), -a))
            toa.append(("generic", False, G.xyzz(a, sa), a))
        for cases, log in ((dbl, 0), (neg, 0), (toa, 0)):
            cases.append(("O", True, G.xyzz(0, junk=i % 2 == 0), log))
    return {"ADD": add, "ADD_AFFINE": aff, "DBL": dbl, "NEG": neg, "TO_AFFINE": toa}


@pytest.mark.parametrize("name", ["G1", "G2"])
def test_additions_and_doubling(harness, tmp_path, name):
    """generic P + Q; P + P and P + (-P) under two scalings (the equality test must see through the representation); O + P, P + O,
    O + O, dbl(O), p at infinity for add_affine, infinity given as zeros and with junk in X, Y; every result also through
    xyzz_to_affine on the device, the results that are O among them"""
    G = GROUPS[name]()
    ops = addition_cases(G)
    order = {op: arrange(cases, G.rnd) for op, cases in ops.items()}
    w = G.w
    out_w = {"ADD": 6 * w, "ADD_AFFINE": 6 * w, "DBL": 6 * w, "NEG": 4 * w, "TO_AFFINE": 2 * w}
    outs = run_family(harness, tmp_path, "add_" + name, [(OP[op], records(order[op]), out_w[op], G.id) for op in order])
    for (op, cases), got in zip(order.items(), outs):
        for lane, (cls, _, _, log) in enumerate(cases):
            what = "%s %s %s, record %d (lane %d)" % (name, op, cls, lane, lane % 64)
            if op == "TO_AFFINE":
                G.check_affine(got[lane], log, what)
                continue
            G.check_xyzz(got[lane, :4 * w], log, what)
            if op != "NEG":
                G.check_affine(got[lane, 4 * w:], log, what + ", to_affine of the result")


def scalars(rnd):
    """[(class, special, k)]: the edges of both double-and-add loops"""
    out = [("k = %s" % n, True, k) for n, k in (("0", 0), ("1", 1), ("2", 2), ("r - 1", R - 1), ("r", R), ("r + 1", R + 1),
                                                  ("2^255", 1 << 255), ("2^256 - 1", (1 << 256) - 1), ("2^224 + 1", (1 << 224) + 1))]
    for j in range(1, 8):   # one bit on each side of every word seam
        out.append(("k = 2^%d" % (32 * j - 1), True, 1 << (32 * j - 1)))
        out.append(("k = 2^%d" % (32 * j), True, 1 << (32 * j)))
    for bits in (20, 32, 64, 100, 128, 200):   # top words zero
        out.append(("k < 2^%d" % bits, True, rnd.getrandbits(bits) | 1 << (bits - 1)))
    out += [("k random below r", False, rnd.randrange(R)) for _ in range(4)]
    out += [("k random below 2^256", False, rnd.getrandbits(256) | 1 << 255) for _ in range(4)]
    return out


@pytest.mark.parametrize("name", ["G1", "G2"])
def test_scalar_multiplications(harness, tmp_path, name):
    """xyzz_mul and xyzz_mul_short: (k mod r) P for 0, 1, 2, r - 1, r, r + 1, 2^255, 2^256 - 1, one bit on each side of every word
    seam, 2^224 + 1 (zero middle words after the accumulator has left infinity: the branch xyzz_mul_short skips only while it is
    at infinity), scalars whose top words are zero, random ones; P scaled and not, and P = O"""
    G = GROUPS[name]()
    ks = scalars(G.rnd)
    pts = G.logs[:8]
    G.need(pts + [k * a for _, _, k in ks for a in pts])
    cases = []
    for cls, special, k in ks:
        kb = k.to_bytes(32, "little")
        for i, a in enumerate(pts):
            cases.append((cls, special, G.xyzz(a, i % 2 == 0) + kb, k * a))
        cases.append((cls, special, G.xyzz(0, junk=special) + kb, 0))
    order = arrange(cases, G.rnd)
    rec = records(order)
    outs = run_family(harness, tmp_path, "mul_" + name, [(OP["MUL"], rec, 4 * G.w, G.id), (OP["MUL_SHORT"], rec, 4 * G.w, G.id)])
    for op, got in zip(("xyzz_mul", "xyzz_mul_short"), outs):
        for lane, (cls, _, _, log) in enumerate(order):
            G.check_xyzz(got[lane], log, "%s %s %s, record %d (lane %d)" % (name, op, cls, lane, lane % 64))
