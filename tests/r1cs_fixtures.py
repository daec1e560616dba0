"""Test helpers of the R1CS check (include/graph_witness_r1cs.h), independent of the C++ loader and kernel:

- write_r1cs: a pure-Python writer of the iden3 binfile "r1cs" v1 format circom writes;
- check / check_constraint: the semantics as big-integer arithmetic, the model the kernel is compared with;
- derive_r1cs: an R1CS derived from a graphgen Builder -- what circom would have kept of the `===` constraints the graph dropped;
- planted_system: random constraint systems that every completed row satisfies by construction.

Constraints are (A, B, C) triples of combinations.  A combination is a {wire: coefficient} dict (written sorted by wire,
coefficients reduced mod r) or a list of (wire, coefficient) pairs (written in the given order, duplicates kept, coefficients
passed through as they are, so a test can write values the loader must refuse).
"""
import contextlib
import struct

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


# -- writer ------------------------------------------------------------------------------------------------------------------
def _lc_bytes(lc):
    items = [(wire, c % R) for wire, c in sorted(lc.items())] if isinstance(lc, dict) else lc
    out = [struct.pack("<I", len(items))]
    for wire, c in items:
        out.append(struct.pack("<I", wire) + c.to_bytes(32, "little"))
    return b"".join(out)


def header_section(n_wires, n_pub_out=0, n_pub_in=0, n_prv_in=0, n_labels=None, n_constraints=0, n8=32, prime=R):
    n_labels = n_wires if n_labels is None else n_labels
    return (struct.pack("<I", n8) + prime.to_bytes(n8, "little") +
            struct.pack("<IIIIQI", n_wires, n_pub_out, n_pub_in, n_prv_in, n_labels, n_constraints))


def constraints_section(constraints):
    return b"".join(_lc_bytes(a) + _lc_bytes(b) + _lc_bytes(c) for a, b, c in constraints)


def map_section(n_wires, labels=None):
    return b"".join(struct.pack("<Q", x) for x in (labels if labels is not None else range(n_wires)))


def container(sections, magic=b"r1cs", version=1):
    """sections: list of (type, payload bytes) in file order"""
    out = [magic, struct.pack("<II", version, len(sections))]
    for t, payload in sections:
        out.append(struct.pack("<IQ", t, len(payload)) + payload)
    return b"".join(out)


def write_r1cs(n_wires, constraints, n_pub_out=0, n_pub_in=0, n_prv_in=0, order=(1, 2, 3)):
    """A valid `.r1cs` image; `order` is the section order in the file."""
    secs = {1: header_section(n_wires, n_pub_out, n_pub_in, n_prv_in, n_constraints=len(constraints)),
            2: constraints_section(constraints), 3: map_section(n_wires)}
    return container([(t, secs[t]) for t in order])


# -- checker ------------------------------------------------------------------------------------------------------------------
def terms(lc):
    """the (wire, coefficient) pairs of a combination in either form"""
    return lc.items() if isinstance(lc, dict) else lc


def _dot(lc, w):
    return sum(c * w[i] for i, c in terms(lc)) % R


def check_constraint(con, w):
    a, b, c = con
    return (_dot(a, w) * _dot(b, w) - _dot(c, w)) % R == 0


def check(constraints, w, indices=None):
    """w: list of ints (one witness row) -> (first failing index or 0xFFFFFFFF, number failing), over `indices` if given."""
    first, n = 0xFFFFFFFF, 0
    for j in (range(len(constraints)) if indices is None else indices):
        if not check_constraint(constraints[j], w):
            n += 1
            first = min(first, j)
    return first, n


MONT_R = (1 << 256) % R           # R mod r: the Montgomery form of 1
MONT_R_INV = pow(1 << 256, -1, R)  # R^-1 mod r
MONT_R2 = (1 << 512) % R          # R^2 mod r


def to_montgomery(x):
    return x * MONT_R % R


def from_montgomery(x):
    return x * MONT_R_INV % R


def row_ints(row):
    """uint8 [W, 32] -> list of ints"""
    b = bytes(row)
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def rows_array(rows):
    """list of rows (lists of ints below 2^256) -> uint8 [B, W, 32]"""
    import numpy as np
    data = b"".join(x.to_bytes(32, "little") for row in rows for x in row)
    return np.frombuffer(data, dtype=np.uint8).reshape(len(rows), len(rows[0]) if rows else 0, 32).copy()


# -- planted systems ----------------------------------------------------------------------------------------------------------
class Planted:
    """A satisfied-by-construction constraint system.  Wires: 0 = the constant 1, then one output wire per constraint that owns
    one (in constraint order), then the zero wire (0 in every row), then the free wires; the last wire is free.

    complete(rnd, fixed=None) -> a row (list of ints below r) satisfying every constraint: free wires random (or `fixed`
    {wire: value}), each output o_j = (A_j B_j - C_j without o_j) / c_o mod r, computed in constraint order."""

    def __init__(self, n_wires, constraints, plan, zero_wire, free):
        self.n_wires, self.constraints, self._plan = n_wires, constraints, plan
        self.zero_wire, self.free = zero_wire, free

    def complete(self, rnd, fixed=None):
        w = [0] * self.n_wires
        w[0] = 1
        for f in self.free:
            w[f] = rnd.randrange(R)
        for f, v in (fixed or {}).items():
            assert f in self.free or f == 0 and v == 1, f
            w[f] = v % R
        for j, out, inv_co, rest in self._plan:
            if out is None:
                continue
            a, b, _ = self.constraints[j]
            w[out] = (_dot(a, w) * _dot(b, w) - _dot(rest, w)) * inv_co % R
        return w


def _pick(rnd, pool):
    c = rnd.choice(pool)
    return rnd.randrange(R) if c is None else c


def planted_system(rnd, n_free, shapes, coef_pool):
    """Constraints from `shapes` (one per constraint, in file order), each a dict:
        a, b, c    lengths of A, B and of C without its output term (c = 0 and out=False: C empty)
        out        True (default): C_j holds an output wire o_j with a nonzero coefficient, at a random position in C
                   False: no output; A then reads only the zero wire (or is empty), so A B = 0, and C must be empty
        dup        duplicate wires: about a quarter of the terms repeat an earlier wire of the same combination, and a side
                   of length >= 3 holds a cancelling pair (w, c), (w, r - c)
        edge       wire 0 and the last wire appear in every side of length >= 2
        pools      (pool_a, pool_b, pool_c) overriding coef_pool per side
    Pools are lists of coefficients; None in a pool is a fresh random field element.  Combinations are lists of
    (wire, coefficient) pairs.  -> Planted."""
    n_out = sum(1 for s in shapes if s.get("out", True))
    zero_wire = 1 + n_out
    free = list(range(zero_wire + 1, zero_wire + 1 + n_free))
    n_wires = zero_wire + 1 + n_free
    last = n_wires - 1
    assert n_free >= 1
    constraints, plan = [], []
    outs = []  # output wires of earlier constraints
    for j, s in enumerate(shapes):
        pools = s.get("pools", (coef_pool,) * 3)
        has_out = s.get("out", True)
        readable = [0, zero_wire] + free + outs

        def side(n, pool, zero_only=False):
            lc = []
            if zero_only:
                for _ in range(n):
                    lc.append((zero_wire, _pick(rnd, pool)))
                return lc
            for i in range(n):
                if s.get("dup") and lc and rnd.random() < 0.25:
                    wire = rnd.choice(lc)[0]
                else:
                    wire = rnd.choice(readable)
                lc.append((wire, _pick(rnd, pool)))
            if s.get("dup") and n >= 3:
                p = rnd.randrange(n - 1)
                wire, c = rnd.choice(readable), rnd.choice((1, 2, rnd.randrange(1, R)))  # 1, r - 1: a +1 / -1 pair
                lc[p], lc[p + 1] = (wire, c), (wire, R - c)
            if s.get("edge") and n >= 2:
                i0, i1 = rnd.sample(range(n), 2)
                lc[i0] = (0, lc[i0][1])
                lc[i1] = (last, lc[i1][1])
            return lc

        a = side(s["a"], pools[0], zero_only=not has_out)
        b = side(s["b"], pools[1])
        rest = side(s["c"], pools[2])
        if has_out:
            out = 1 + len(outs)
            co = 0
            while co % R == 0:
                co = _pick(rnd, pools[2])
            c = list(rest)
            c.insert(rnd.randrange(len(c) + 1), (out, co))
            plan.append((j, out, pow(co, -1, R), rest))
            outs.append(out)
        else:
            assert not rest, "a constraint without an output wire has an empty C"
            c = []
            plan.append((j, None, None, None))
        constraints.append((a, b, c))
    return Planted(n_wires, constraints, plan, zero_wire, free)


# -- derivation from a graphgen Builder --------------------------------------------------------------------------------------
_MAX_TERMS = 600


def _lin_add(x, y, s=1):
    out = dict(x)
    for k, v in y.items():
        out[k] = (out.get(k, 0) + s * v) % R
    return {k: v for k, v in out.items() if v}


def _lin_scale(x, k):
    k %= R
    return {w: v * k % R for w, v in x.items() if v * k % R}


# An expression cut at wires: ("lin", L) = linear form over wires (wire 0 = the constant 1), or ("quad", La, Lb, L) = La * Lb + L.
def _combine(op, xs):
    if any(x is None for x in xs):
        return None
    if op == "Neg":
        x = xs[0]
        return ("lin", _lin_scale(x[1], -1)) if x[0] == "lin" else ("quad", _lin_scale(x[1], -1), x[2], _lin_scale(x[3], -1))
    x, y = xs
    if op in ("Add", "Sub"):
        s = 1 if op == "Add" else -1
        if x[0] == "quad" and y[0] == "quad":
            return None
        if y[0] == "quad":
            if s == -1:
                y = ("quad", _lin_scale(y[1], -1), y[2], _lin_scale(y[3], -1))
            return ("quad", y[1], y[2], _lin_add(y[3], x[1]))
        if x[0] == "quad":
            return ("quad", x[1], x[2], _lin_add(x[3], y[1], s))
        r = _lin_add(x[1], y[1], s)
        return ("lin", r) if len(r) <= _MAX_TERMS else None
    if op == "Mul":
        const = lambda e: e[0] == "lin" and set(e[1]) <= {0}
        if const(x) or const(y):
            k, e = (x[1].get(0, 0), y) if const(x) else (y[1].get(0, 0), x)
            if e[0] == "lin":
                return ("lin", _lin_scale(e[1], k))
            return ("quad", _lin_scale(e[1], k), e[2], _lin_scale(e[3], k))
        if x[0] == "lin" and y[0] == "lin":
            return ("quad", x[1], y[1], {})
        return None
    return None  # Div, bit operations, comparisons, TernCond, ...: `<--` hints


def _wire_lc(x, wire_of, forms):
    """linear form of node x cut at wires, or None"""
    if x in wire_of:
        return {wire_of[x]: 1}
    f = forms[x]
    return f[1] if f is not None and f[0] == "lin" else None


@contextlib.contextmanager
def gadget_constraints():
    """While building a circuit inside this context, circomlib's explicit constraints of the gadgets the generator names are
    recorded on the Builder (b._r1cs_gadgets): Num2Bits (bit * (bit - 1) = 0, sum bit * 2^i = in) and IsZero (in * out = 0)."""
    import cwc_import
    C = cwc_import.load().graphgen.circuits
    orig_n2b, orig_isz = C.num2bits, C.is_zero

    def num2bits(b, x, n, signals=True):
        bits = orig_n2b(b, x, n, signals)
        if signals:
            b.__dict__.setdefault("_r1cs_gadgets", []).append(("num2bits", x, list(bits)))
        return bits

    def is_zero(b, x):
        out = orig_isz(b, x)
        b.__dict__.setdefault("_r1cs_gadgets", []).append(("is_zero", x, out))
        return out

    C.num2bits, C.is_zero = num2bits, is_zero
    try:
        yield
    finally:
        C.num2bits, C.is_zero = orig_n2b, orig_isz


def derive_r1cs(b, extra=()):
    """-> list of (A, B, C) constraints over the Builder's witness list (wire i = b._witness[i]; wire 0 = Input(0) = 1).

    Every witness signal whose defining expression, cut at wires, is at most quadratic in wires and constants (Add, Sub, Mul,
    Neg, constants only) gets `La * Lb = w - L` (a linear one `0 * 0 = ... - (w - L)`); a node listed twice gets `w' = w`.
    Other signals are `<--` hints and get no constraint.  Then the gadget constraints recorded by gadget_constraints() whose
    operands are expressible, then `extra` ((A, B, C) over node handles: {node: coefficient}, node -1 = the constant 1)."""
    sym = b._sym
    wire_of = {}
    dup = []
    for i, node in enumerate(b._witness):
        if node in wire_of:
            dup.append((wire_of[node], i))
        else:
            wire_of[node] = i
    forms = [None] * len(sym)
    for s, t in enumerate(sym):
        k = t[0]
        if k == "Const":
            forms[s] = ("lin", {0: t[1] % R} if t[1] % R else {})
        elif k == "Input":
            forms[s] = ("lin", {0: 1}) if t[1] == 0 else None  # a main input is only an expression through its wire
        else:
            ops = t[2:]
            xs = [("lin", {wire_of[o]: 1}) if o in wire_of else forms[o] for o in ops]
            forms[s] = _combine(t[1], xs)
    cons = []
    for node, w in sorted(wire_of.items(), key=lambda kv: kv[1]):
        t = sym[node]
        if t[0] in ("Const", "Input"):
            continue
        f = forms[node]
        if f is None:
            continue
        if f[0] == "lin":
            cons.append(({}, {}, _lin_add({w: 1}, f[1], -1)))
        else:
            cons.append((dict(f[1]), dict(f[2]), _lin_add({w: 1}, f[3], -1)))
    for w0, w1 in dup:
        cons.append(({}, {}, {w1: 1, w0: R - 1}))
    for g in b.__dict__.get("_r1cs_gadgets", ()):
        if g[0] == "num2bits":
            _, x, bits = g
            lx = _wire_lc(x, wire_of, forms)
            if any(bt not in wire_of for bt in bits):
                continue
            for bt in bits:
                cons.append(({wire_of[bt]: 1}, {wire_of[bt]: 1, 0: R - 1}, {}))
            if lx is not None:
                s = {}
                for i, bt in enumerate(bits):
                    s = _lin_add(s, {wire_of[bt]: pow(2, i, R)})
                cons.append(({}, {}, _lin_add(s, lx, -1)))
        else:
            _, x, out = g
            lx = _wire_lc(x, wire_of, forms)
            if lx is not None and out in wire_of:
                cons.append((lx, {wire_of[out]: 1}, {}))
    for abc in extra:
        cons.append(tuple({(0 if n == -1 else wire_of[n]): c % R for n, c in lc.items()} for lc in abc))
    return cons
