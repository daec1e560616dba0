"""Fixtures of tests/test_gpu_groth16_msm.py and tests/test_msm_model_host.py: a known-log proving key that costs seconds at any
size, the two section-4 shapes that make the quotient h known in closed form, and the scalar rows that drive the prover's MSM
(r1cs/msm.hip) to each digit event and chunk event of tests/msm_model.py at every window width.

TiledKnownLog: as groth16_fixtures.KnownLog every base list is an arithmetic progression of known logs, but of P points only,
repeated to the list's length (the point bytes are tiled as bytes), so base i has the log of point i mod P and bases i and
i + P are equal.  P = 1031: at least 1024, so an MSM's additions are overwhelmingly generic ones, and a prime, so no
multiple of any bucket count n_b = 2^(c-1); a bucket sweep (scalar of wire i: (i mod n_b) + 1) then puts a different set
of points into every bucket.
"""
import random

from tests import groth16_fixtures as GF
from tests import msm_model as M
from tests import qap_reference as QR
from tests import r1cs_fixtures as F
from tests import zkey_coefs_fixtures as ZF

R = GF.R
P = 1031
N_PUB = 3
# scalars per row (nVars + 2) of the wire-side keys: 2^(c+3) for c = 8 .. 15, and both sides of the first and the last step of c
WIRE_SIZES = (2047, 2048, 4096, 8192, 16384, 32768, 65536, 131072, 262143, 262144)
H_POWERS = tuple(range(11, 19))   # domains of the H-side keys: c = 8 .. 15 in the H MSM
H_N_VARS = 40                     # their wire MSMs run at c = 7
PLANTED_POWERS = (11, 12)
LISTS = ("a", "b1", "b2", "c", "h")


class TiledKnownLog:
    """A zkey of tiled progressions (not a valid setup): every MSM's discrete log is a dot product with logs[name][i mod P].
    tweak(key), called before the key is written, may call key.set_infinity(name, indices): those bases become the point at
    infinity (log 0).  entries: section 4 as (matrix, constraint, signal, value)."""

    def __init__(self, n_vars, n_public, domain_size, entries, seed=3, tweak=None):
        rnd = random.Random(seed)
        self.n_vars, self.n_pub, self.n = n_vars, n_public, domain_size
        self.alpha, self.beta, self.delta, self.gamma = (rnd.randrange(1, R) for _ in range(4))
        self.size = {"a": n_vars, "b1": n_vars, "b2": n_vars, "c": n_vars - n_public - 1, "h": domain_size}
        self.logs, self.inf, data = {}, {k: set() for k in LISTS}, {}
        for name in LISTS:
            curve, enc, width = (GF.G2, GF.g2_bytes, 128) if name == "b2" else (GF.G1, GF.g1_bytes, 64)
            pts, self.logs[name] = GF.progression(curve, rnd.randrange(R), rnd.randrange(R), P)
            assert None not in pts and len(set(pts)) == P
            tile = b"".join(map(enc, pts))
            data[name] = bytearray((tile * (self.size[name] // P + 1))[:self.size[name] * width])
        if tweak:
            tweak(self)
        for name in LISTS:
            width = 128 if name == "b2" else 64
            for i in self.inf[name]:
                data[name][i * width:(i + 1) * width] = bytes(width)
        g1 = GF.G1.gen_muls([self.alpha, self.beta, self.delta])
        g2 = GF.G2.gen_muls([self.beta, self.gamma, self.delta])
        frame = GF.write_zkey(n_vars, n_public, domain_size, g1[0], g1[1], g2[0], g2[1], g1[2], g2[2], [None] * (n_public + 1), [], [], [], [], [])
        body = {4: ZF.section4(entries), 5: bytes(data["a"]), 6: bytes(data["b1"]), 7: bytes(data["b2"]), 8: bytes(data["c"]), 9: bytes(data["h"])}
        self.zkey = ZF.join([(i, body.get(i, b)) for i, b in ZF.sections(frame)])

    def set_infinity(self, name, indices):
        assert all(0 <= i < self.size[name] for i in indices)
        self.inf[name].update(indices)

    def dot(self, name, scalars):
        """sum scalars[i] log(base i) mod r over the list `name` (scalars aligned with its first base)"""
        assert len(scalars) == self.size[name]
        logs = self.logs[name]
        acc = sum(sum(scalars[j::P]) * logs[j] for j in range(min(P, len(scalars))))
        acc -= sum(scalars[i] * logs[i % P] for i in self.inf[name])
        return acc % R

    def proof_logs(self, w, h_log, r, s):
        """(a, b, c) logs of the proof of row w; h_log: the log of the H MSM (dot('h', h), or its closed form)"""
        w = [x % R for x in w]
        a = (self.alpha + self.dot("a", w) + r * self.delta) % R
        b = (self.beta + self.dot("b2", w) + s * self.delta) % R
        b1 = (self.beta + self.dot("b1", w) + s * self.delta) % R
        c = (self.dot("c", w[self.n_pub + 1:]) + h_log + s * a + r * b1 - r * s * self.delta) % R
        return a, b, c

    want_bytes = GF.Trapdoor.want_bytes


# -- section 4 ----------------------------------------------------------------------------------------------------------------
ZERO_QUOTIENT = [(0, 0, 0, 1)]   # a_0 = w_0 and b = 0: h = 0 for any witness


def constant_quotient(p):
    """A(x) = w_0 x, B(x) = w_0 x^(n-1) on the domain of n = 2^p points, so C = w_0^2 and h_j = w_0^2 (g^n - 1) = -2 w_0^2 at every
    coset point: with w_0 = 1 every h scalar is r - 2"""
    n = 1 << p
    wn, _ = QR.roots(p)
    wi = pow(wn, -1, R)
    out, x, y = [], 1, 1
    for k in range(n):
        out.append((0, k, 0, x))
        out.append((1, k, 0, y))
        x, y = x * wn % R, y * wi % R
    return out


# -- scalar rows --------------------------------------------------------------------------------------------------------------
def edge_scalars(shape):
    """-> (scalars, expected): scalars that put each digit event of the recoding into window 0, a middle window, the window
    before the top and the top window, wherever the scalar stays below r; expected[event] = the windows reached (for the
    counted events: how many scalars were placed).  Every value follows from c and r alone."""
    c, n_b, n_win = shape.c, shape.n_b, shape.n_win
    top, full = n_win - 1, (1 << c) - 1
    out = [0, 1, R - 1, 1 << 253, (1 << 253) - 1]
    expected = {e: set() for e in M.DIGIT_EVENTS}
    expected.update(carry_chain=0, top_max=0, top_max_carry=0, zero_scalar=1)

    def put(k, event=None, win=None):
        if not 0 <= k < R:
            return False
        out.append(k)
        if event in M.DIGIT_EVENTS:
            expected[event].add(win)
        elif event:
            expected[event] += 1
        return True

    for w in sorted({0, n_win // 2, n_win - 2, top}):
        s = c * w
        put(n_b << s, "top_bucket", w)                               # digit +n_b
        put((n_b + 1) << s, "most_negative", w)                      # digit -(n_b - 1), carry out
        if w:
            carry = (n_b + 1) << (s - c)                             # window w - 1 carries into w
            put(((n_b - 1) << s) | carry, "top_bucket_by_carry", w)  # n_b - 1 with a carry in: +n_b again
            put((full << s) | carry, "zero_with_carry", w)           # digit 0, and the carry moves on
    s = c * top
    put((1 << s) - 1, "carry_chain")                                  # all ones below the top window: -1, 0, ..., 0, +1
    put((1 << s) | ((1 << s) - 1), "carry_chain")
    top_max, top_carry = M.top_values(shape)
    assert put(top_max << s, "top_max")
    assert put((top_carry << s) | ((n_b + 1) << (s - c)), "top_max_carry")
    for w in range(n_win):
        if M.straddles(c, w):
            put((n_b + 1) << (c * w), "straddle", w)                  # the window's lowest and highest bit
            put(((n_b >> 1) | 1) << (c * w))
    return out, expected


def wire_rows(shape, n_vars, seed, infinity=(), ones=False):
    """-> [(class name, scalars of the n_vars wires)] for one wire-side key"""
    assert shape.n_sc == n_vars + 2
    rnd = random.Random(seed)
    c, n_b, mid = shape.c, shape.n_b, shape.n_win // 2
    edges, _ = edge_scalars(shape)
    rows = [("uniform", [rnd.randrange(R) for _ in range(n_vars)]),
            ("digit edges", [edges[i % len(edges)] for i in range(n_vars)]),
            ("skew", [(1 if rnd.random() < 0.5 else 0) if rnd.random() < 0.95 else rnd.randrange(R) for _ in range(n_vars)])]
    for w in (0, mid):
        sweep = [((i % n_b) + 1) << (c * w) for i in range(n_vars)]
        # the wires outside the C MSM name a bucket of another window, where the row has nothing else: runs of skipped entries
        sweep[:N_PUB + 1] = [(i + 2) << (c * (w + 2)) for i in range(N_PUB + 1)]
        rows.append(("bucket sweep, window %d" % w, sweep))
        rows.append(("bucket sweep, window %d, negated" % w, [R - x for x in sweep]))
    rows.append(("single bucket n_b", [n_b] * n_vars))
    rows.append(("single bucket n_b 2^c + 1", [(n_b << c) + 1] * n_vars))
    rows.append(("cancellation and doubling", cancel_row(shape, n_vars, rnd)))
    if infinity:
        row = [rnd.randrange(R) for _ in range(n_vars)]
        for j, i in enumerate(sorted(infinity)):
            row[i] = (5 + j) if j % 2 else ((1 << c) - 5 - j)   # a positive and a negative digit in window 0
        rows.append(("infinity bases", row))
    if ones:
        rows.append(("all ones", [1] * n_vars))
    return rows


CANCEL_WIRES = 10


def cancel_row(shape, n_vars, rnd):
    """zeros, and on wires i, i + P (equal bases): +d and -d in one bucket (P + (-P) in xyzz_add_affine), +d and +d (its
    doubling), +d, +d, -d over i, i + P, i + 2 P (where the row is long enough), and k with r - k, whose digits may join a named bucket:
    the census counts the buckets that hold their pair alone"""
    c, row = shape.c, [0] * n_vars
    assert n_vars > N_PUB + 1 + 4 * CANCEL_WIRES * 2 + P and 6 * CANCEL_WIRES + 2 < shape.n_b
    i, d = N_PUB + 1, 2
    for w in (0, shape.n_win // 2):
        s = c * w
        for _ in range(CANCEL_WIRES):
            row[i], row[i + P] = d << s, ((1 << c) - d) << s            # digits +d and -d (the second one carries a +1 upward)
            row[i + 1], row[i + 1 + P] = (d + 1) << s, (d + 1) << s     # +d, +d
            if i + 2 + 2 * P < n_vars:
                row[i + 2], row[i + 2 + P], row[i + 2 + 2 * P] = (d + 2) << s, (d + 2) << s, ((1 << c) - d - 2) << s
            k = rnd.randrange(R)
            row[i + 3], row[i + 3 + P] = k, R - k
            i, d = i + 4, d + 3
    return row


def rs_pairs(n, seed):
    rnd = random.Random(seed)
    fixed = [(0, 0), (R - 1, R - 1), (1, R - 1)]
    return (fixed + [(rnd.randrange(R), rnd.randrange(R)) for _ in range(n)])[:n]


def class_rs(names, seed):
    """(r, s) of the wire-side rows.  r and s are scalars of the same lists as the wires, so the rows built to hold one kind of
    digit or run alone get (0, 0), which adds no entry; the edge pairs and the random ones ride on the rows of random scalars"""
    rnd = random.Random(seed)
    fixed = {"skew": (R - 1, R - 1), "cancellation and doubling": (1, R - 1)}
    return [fixed.get(name, (rnd.randrange(R), rnd.randrange(R)) if name in ("uniform", "infinity bases") else (0, 0)) for name in names]


def infinity_wires(n_vars):
    """wires whose A, B1, B2 and C bases are set to infinity: inside the C range, one with an equal-base partner, the last one"""
    return (N_PUB + 1, 100, 101, 100 + P, n_vars // 2, n_vars - 1)


def wire_case(n_sc):
    """-> (shape, n_vars, tweak or None, [(class, scalars)], [(r, s)]) of one wire-side size; the same lists on the host (census)
    and on the GPU"""
    shape = M.msm_shape(n_sc)
    n_vars = n_sc - 2
    inf = infinity_wires(n_vars) if n_sc in (4096, 262144) else ()
    rows = wire_rows(shape, n_vars, 1000 + n_sc, infinity=inf, ones=n_sc in (2048, 262144))
    return shape, n_vars, inf, rows, class_rs([name for name, _ in rows], n_sc)


def wire_tweak(inf):
    def tweak(key):
        for name in ("a", "b1", "b2"):
            key.set_infinity(name, inf)
        key.set_infinity("c", [i - N_PUB - 1 for i in inf])
    return tweak if inf else None


def batch5_rows(shape, n_vars, seed):
    """the uniform and digit-edge classes as a batch of five rows (the edges rotated, so a wire meets another edge per row)"""
    rnd = random.Random(seed)
    edges, _ = edge_scalars(shape)
    return [("uniform" if j % 2 == 0 else "digit edges",
             [rnd.randrange(R) for _ in range(n_vars)] if j % 2 == 0 else [edges[(i + 7 * j) % len(edges)] for i in range(n_vars)]) for j in range(5)]


def scalar_lists(rows, rs):
    """wire rows and their (r, s) -> the scalar lists of the wire MSMs (the wires, then r and s)"""
    return [list(w) + [r_, s_] for (_, w), (r_, s_) in zip(rows, rs)]


def h_rows(seed, n=2):
    """rows of the H-side keys: wire 0 = 1, every other wire random"""
    rnd = random.Random(seed)
    return [[1] + [rnd.randrange(R) for _ in range(H_N_VARS - 1)] for _ in range(n)]


def h_infinity(p):
    return (0, 5, P + 5, (1 << p) - 1) if p in (12, 18) else ()


def planted_case(p):
    """a planted system (r1cs_fixtures) that fills the domain of 2^p -> (planted, shuffled section-4 entries, three satisfying rows,
    their h by qap_reference.h_of: uniform below r)"""
    rnd = random.Random(300 + p)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range((1 << p) - N_PUB - 1 - 5)]
    pl = F.planted_system(rnd, 6, shapes, [1, R - 1, 2, F.MONT_R, None])
    ent = ZF.entries_of(pl.constraints, N_PUB)
    rnd.shuffle(ent)
    rows = [pl.complete(rnd) for _ in range(3)]
    return pl, ent, rows, [QR.h_of(pl.constraints, N_PUB, w) for w in rows]
