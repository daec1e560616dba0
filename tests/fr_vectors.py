"""Operand sets that drive the field primitives (csrc/fr_gfx950.hpp, r1cs/fq_gfx950.hpp) into the states where a carry or
a borrow decides, built deterministically from a seed.

Lane-cooperative sequences (K = 4: fr_mul_coop4, fr_mul_coop4r, fr_addsub_coop4).  tools/codegen/gen_fr_mul_coop.py's
emulator is the observer: `Coop4.run` steps the scheduled instruction list and reads the scalar masks at the two
s_xor_b64 (carry / borrow resolution) and at the final SEL.  Per group of four lanes (lane k holds bits [64k, 64k + 64)):

  carry       a non-top lane has P set (its 64 bits are all ones after the first pass) and a carry coming in
  borrow1     borrow pass: exactly one non-top lane has P set (W_k == r_k) and a borrow coming in
  borrow2     borrow pass: lanes 1 and 2 both, the borrow generated in lane 0
  sel_prop_lt the borrow reached the top lane only through propagating lane 2 and the top lane borrowed: W < r
  sel_prop_ge the same borrow, absorbed by the top lane (W_3 > r_3): W >= r
  sel_first_lt / sel_first_ge  decided by the first pass alone (top lane's own borrow / no borrow reaching the top lane)

The borrow pass works on the normalised value W (the product before its conditional subtraction, a + b, or a - b + r), so
those operands are constructed: W is chosen and the operands solved for (products: u = (a b + m r) / 2^256 is unique for
a, b; b = W 2^256 / a mod r and the pairs that give u = W are kept).  The carry pass works on the unnormalised words of the
lanes; for products it is searched (results whose lane 1 wrapped to almost zero and whose lane 2 is zero: all ones + carry is one
of the two ways to get there),
for additions and subtractions it is constructed from the lanes' own sums.  Whatever the construction, only what the
emulator shows is counted.

One-lane sequences (fr_mul, fr_mul_wave, fr_sqr, fr_to_mont, fr_from_mont, fr_add/sub and their _wave forms, fq_*): no
emulator exists, the vectors come from the mathematics: u = (a b + m r) / 2^256 with m = -a b / r mod 2^256 is unique, so
operands are chosen by u."""
import functools
import importlib.util
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _load("gen_fr_mul_coop", os.path.join(ROOT, "tools", "codegen", "gen_fr_mul_coop.py"))

R = gen.P_INT
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
B256 = 1 << 256
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
ADD, SUB, MUL = 0, 1, 2   # program_dev.h SUB_ADD / SUB_SUB / SUB_MULT
KIND_NAME = {ADD: "add", SUB: "sub", MUL: "mul"}
SEQS = {"mul": (False, False), "mulr": (True, False), "lin": (True, True)}   # name -> (riders, lin_only)
SEQ_KINDS = {"mul": (MUL,), "mulr": (MUL, ADD, SUB), "lin": (ADD, SUB)}
IDLE = {"mul": (0, 0, MUL), "mulr": (0, 0, MUL), "lin": (0, 0, SUB)}  # zero operands, as the interpreter's idle groups
EVENTS = ("carry", "borrow1", "borrow2", "sel_prop_lt", "sel_prop_ge", "sel_first_lt", "sel_first_ge")
LOUD = frozenset(EVENTS[:5])   # what makes a neighbour "eventful"
RIDER_CLASSES = {ADD: ("add_rm1", "add_r", "add_rp1", "add_run"), SUB: ("sub_eq", "sub_m1", "sub_lt", "sub_run")}
MUTANTS = ("carry_p_zero", "borrow_p_zero", "top_kept", "top_kept_carry", "sel_first_only")


def lane(x, k):
    return (x >> (64 * k)) & M64


def mont_u(a, b, mod=R):
    """the value before the final conditional subtraction of a word-serial Montgomery product"""
    m = (-a * b * pow(mod, -1, B256)) % B256
    return (a * b + m * mod) >> 256


def want(a, b, kind, mod=R):
    return a * b * pow(B256, -1, mod) % mod if kind == MUL else (a + b) % mod if kind == ADD else (a - b) % mod


# ---- the emulator as an observer -----------------------------------------------------------------------------------------
class Coop4:
    def __init__(self, seq, mutant=None):
        self.seq = seq
        riders, lin_only = SEQS[seq]
        self.riders, self.lin_only = riders, lin_only
        self.p, _, _ = gen.make(4, riders=riders, lin_only=lin_only)
        self.p.schedule()
        ins = self.p.ins
        self.xor = [i for i, x in enumerate(ins) if x.text.startswith("s_xor_b64")]
        self.sel = [i for i, x in enumerate(ins) if x.text.startswith("s_or_b64") and "%[sb]" in x.sr]
        andn = [i for i, x in enumerate(ins) if x.text.startswith("s_andn2_b64") and "%[top]" in x.sr]
        pm = [i for i in andn if ins[i].sw == ("%[sp]",)]
        assert len(self.xor) == 2 and len(self.sel) == 1 and len(andn) == 4 and len(pm) == 2 and pm[0] < self.xor[0] < pm[1] < self.xor[1]
        self.X, self.SEL, self.G = ins[self.xor[0]].sw[0], ins[self.sel[0]].sw[0], [r for r in ins[self.sel[0]].sr if r != "%[sb]"][0]

        def zero_p(st):
            st.s["%[sp]"] = 0

        def keep(i):
            d, a = ins[i].sw[0], ins[i].sr[0]

            def fn(st):
                st.s[d] = st.s[a]
            return fn

        def first_only(st):
            st.s[self.SEL] = st.s["%[sb]"]
        if mutant == "carry_p_zero":
            ins[pm[0]].fn = zero_p
        elif mutant == "borrow_p_zero":
            ins[pm[1]].fn = zero_p
        elif mutant == "top_kept":
            for i in andn:
                ins[i].fn = keep(i)
        elif mutant == "top_kept_carry":
            for i in andn:
                if i < self.xor[0]:
                    ins[i].fn = keep(i)
        elif mutant == "sel_first_only":
            ins[self.sel[0]].fn = first_only
        else:
            assert mutant is None, mutant

    def run(self, ops):
        """ops: 16 x (a, b, kind).  Returns (results, events): the 16 values the lanes return and, per group, the set of
        event names the masks show."""
        assert len(ops) == 16
        st = gen.St()
        A, Bv, kinds = [o[0] for o in ops], [o[1] for o in ops], [o[2] for o in ops]
        for i in range(8):
            st.v["%%[a%d]" % i] = [(A[l // 4] >> (32 * i)) & M32 for l in range(64)]
        for j in range(2):
            st.v["%%[b%d]" % j] = [(Bv[l // 4] >> (32 * ((l % 4) * 2 + j))) & M32 for l in range(64)]
            st.v["%%[aq%d]" % j] = [(A[l // 4] >> (32 * ((l % 4) * 2 + j))) & M32 for l in range(64)]
            st.v["%%[n%d]" % j] = [gen.P_LIMBS[(l % 4) * 2 + j] for l in range(64)]
        st.s["%[inv]"] = gen.INV32
        st.s["%[top]"] = gen.top_mask(4)
        st.s["%[lane0]"] = sum(1 << i for i in range(0, 64, 4))
        st.v["%[sub]"] = [kinds[l // 4] for l in range(64)]
        seen = {}
        for i, x in enumerate(self.p.ins):
            if i in self.xor:
                pmask, gen0 = st.s["%[sp]"], st.s[self.X]
                x.fn(st)
                seen[i] = (pmask, gen0, st.s[self.X])
            elif i == self.sel[0]:
                seen["sel"] = (st.s["%[sb]"], st.s[self.G])
                x.fn(st)
            else:
                x.fn(st)
        out, events = [], []
        pc, _, xc = seen[self.xor[0]]
        pb, gb, xb = seen[self.xor[1]]
        b1, g2 = seen["sel"]
        for g in range(16):
            got = 0
            for k in range(4):
                for j in range(2):
                    got |= st.v["%%[r%d]" % j][4 * g + k] << (32 * (2 * k + j))
            out.append(got)

            def bits(m):
                return (m >> (4 * g)) & 15
            ev = set()
            if bits(pc & xc) & 7:
                ev.add("carry")
            hit = bits(pb & xb) & 7
            if hit == 6:
                ev.add("borrow2")
            elif hit in (1, 2, 4):
                ev.add("borrow1")
            top_in, g_2, b1t, g2t = bits(xb) & 8, bits(gb) & 4, bits(b1) & 8, bits(g2) & 8
            if top_in and not g_2 and not b1t:
                ev.add("sel_prop_lt" if g2t else "sel_prop_ge")
            if b1t and not g2t:
                ev.add("sel_first_lt")
            if not b1t and not top_in:
                ev.add("sel_first_ge")
            if top_in:
                ev.add("top_borrow_in")
            events.append(ev)
        return out, events


def rider_classes(op, ev):
    """the classes of the issue's rider list an operand triple belongs to (plain arithmetic + the emulator's events)"""
    a, b, kind = op
    c = set()
    if kind == ADD:
        for name, s in (("add_rm1", R - 1), ("add_r", R), ("add_rp1", R + 1)):
            if a + b == s:
                c.add(name)
        if "carry" in ev:   # lane 0's sum overflows into lane 1, which wraps and generates; lane 2 propagates into the top lane
            c.add("add_run")
    if kind == SUB:
        if a == b:
            c.add("sub_eq")
        if a == b - 1:
            c.add("sub_m1")
        if a < b:
            c.add("sub_lt")
        if "borrow2" in ev and "top_borrow_in" in ev:   # borrow generated in lane 0, through lanes 1 and 2 into the top lane
            c.add("sub_run")
    return c


# ---- operands for a chosen W -------------------------------------------------------------------------------------------------
def solve_mul(w, rnd, a_limit=R, tries=200):
    """(a, b) with a < a_limit, b < r and (a b + m r) / 2^256 == w, or None"""
    t = w % R
    for _ in range(tries):
        a = rnd.randrange(1, a_limit) if w >= R or rnd.random() < 0.7 else rnd.randrange(1, 1 << rnd.choice([64, 128, 200]))
        if a % R == 0:
            continue
        b = t * B256 * pow(a, -1, R) % R
        if mont_u(a, b) == w:
            return a, b
    return None


def solve(w, kind, rnd):
    """operands of `kind` whose normalised value in front of the subtraction of r is w (0 <= w < 2r)"""
    if kind == MUL:
        ab = solve_mul(w, rnd)
        return None if ab is None else (ab[0], ab[1], MUL)
    if kind == ADD:   # a + b = w
        lo, hi = max(0, w - R + 1), min(R - 1, w)
        if lo > hi:
            return None
        a = rnd.randint(lo, hi)
        return a, w - a, ADD
    # a - b + r = w
    lo, hi = max(0, R - w), min(R - 1, 2 * R - 1 - w)   # range of b with 0 <= a = w - r + b < r
    if lo > hi:
        return None
    b = rnd.randint(lo, hi)
    return w - R + b, b, SUB


def borrow_targets(rnd):
    """values W in [0, 2r) by the lane pattern of W - r: per class a list of generators"""
    r = [lane(R, k) for k in range(4)]

    def join(l):
        return sum(v << (64 * k) for k, v in enumerate(l))

    def below(k):
        return rnd.choice([r[k] - 1, 0, rnd.randrange(r[k]), r[k] - rnd.randrange(1, 1 << 32)])

    def above(k):
        return rnd.choice([r[k] + 1, rnd.randrange(r[k] + 1, 1 << 64), M64]) if k < 3 else rnd.choice([r[3] + 1, rnd.randrange(r[3] + 1, 2 * r[3])])

    def anyl(k):
        return rnd.randrange(1 << 64) if k < 3 else rnd.randrange(2 * r[3])
    t = {
        "borrow2": lambda: join([below(0), r[1], r[2], rnd.choice([r[3], above(3), below(3)])]),
        "borrow1": lambda: rnd.choice([join([anyl(0), below(1), r[2], anyl(3)]), join([below(0), r[1], above(2), anyl(3)]),
                                       join([below(0), r[1], below(2), anyl(3)])]),
        "sel_prop_lt": lambda: join([rnd.choice([below(0), anyl(0)]), rnd.choice([below(1), r[1]]), r[2], r[3]]),
        "sel_prop_ge": lambda: join([rnd.choice([below(0), anyl(0)]), rnd.choice([below(1), r[1]]), r[2], above(3)]),
        "sel_first_lt": lambda: join([anyl(0), anyl(1), anyl(2), below(3)]),
        "sel_first_ge": lambda: rnd.choice([join([anyl(0), anyl(1), above(2), rnd.choice([r[3], above(3)])]), R, R + 1, join([r[0], r[1], r[2], above(3)])]),
    }
    return t


def carry_candidate(kind, rnd):
    """operands that may show a carry into an all-ones lane (lane 2; see test_fr_primitives_host.py for why only there)"""
    r = [lane(R, k) for k in range(4)]
    if kind == MUL:   # searched: a result whose lane 2 is zero came either from 0 or from all ones + carry
        w = rnd.randrange(1 << 64) | (rnd.randrange(3) << 64) | (rnd.randrange(2 * r[3]) << 192)   # (lane 1 wrapped: it generated)
        if w >= 2 * R:
            return None
        ab = solve_mul(w, rnd, tries=20)
        return None if ab is None else (ab[0], ab[1], MUL)
    if kind == ADD:   # lane sums: lane 0 overflows, lanes 1 and 2 are all ones
        a = [rnd.randrange(1, 1 << 64), rnd.randrange(1 << 64), rnd.randrange(1 << 64), rnd.randrange(r[3] - 1)]
        b = [rnd.randrange((1 << 64) - a[0], 1 << 64), M64 - a[1], M64 - a[2], rnd.randrange(r[3] - 1)]
    else:             # a_k + r_k + ~b_k (+ 1 in lane 0): lane 0 overflows once, lanes 1 and 2 give all ones
        b = [rnd.randrange(1 << 64), rnd.randrange(r[1], 1 << 64), rnd.randrange(r[2], 1 << 64), rnd.randrange(r[3] - 1)]
        a = [rnd.randrange(max(0, b[0] - r[0]), min(1 << 64, (1 << 64) + b[0] - r[0])), b[1] - r[1], b[2] - r[2], rnd.randrange(r[3] - 1)]
    av, bv = sum(v << (64 * k) for k, v in enumerate(a)), sum(v << (64 * k) for k, v in enumerate(b))
    return (av, bv, kind) if av < R and bv < R else None


def rider_candidates(kind, rnd):
    out = []
    if kind == ADD:
        for s in (R - 1, R, R + 1):
            out.append(solve(s, ADD, rnd))
    else:
        b = rnd.randrange(1, R)
        out += [(b, b, SUB), (b - 1, b, SUB), (0, b, SUB), (0, R - 1, SUB), (0, 1, SUB), (rnd.randrange(b), b, SUB), (R - 1, R - 1, SUB)]
    return out


# ---- the vector set of one sequence ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build(seq, seed=20261016, pool_size=6):
    """-> {"waves": [16 x (a, b, kind)], "quiet": set of wave indices made of one class with idle neighbours, "pool": ...}.
    Every wave is a full wavefront of the sequence: 16 groups of four lanes."""
    rnd = random.Random("%s-%d" % (seq, seed))
    emu = Coop4(seq)
    kinds = SEQ_KINDS[seq]
    pool = {}   # (class, kind) -> [op]

    def classify(cands):
        cands = [c for c in cands if c is not None]
        for i in range(0, len(cands), 16):
            chunk = cands[i:i + 16]
            ops = chunk + [IDLE[seq]] * (16 - len(chunk))
            res, evs = emu.run(ops)
            for op, got, ev in zip(chunk, res, evs):
                assert got == want(*op), (seq, op, got)
                for c in (ev & set(EVENTS)) | rider_classes(op, ev):
                    lst = pool.setdefault((c, op[2]), [])
                    if len(lst) < pool_size and op not in lst:
                        lst.append(op)
    tg = borrow_targets(rnd)
    for kind in kinds:
        for _ in range(3):
            cands = [solve(tg[c](), kind, rnd) for c in tg for _ in range(3)]
            if kind != MUL:
                cands += rider_candidates(kind, rnd)
            classify(cands)
        for _ in range(60):   # the carry pass: constructed for the linear kinds, searched for products
            if len(pool.get(("carry", kind), [])) >= pool_size:
                break
            classify([carry_candidate(kind, rnd) for _ in range(16)])
    keys = sorted(pool)
    waves, quiet = [], set()
    # (1) quiet neighbours: one class per wave in four positions, every other group idle
    for key in keys:
        for shift in range(4):
            ops = [IDLE[seq]] * 16
            for p in range(shift, 16, 4):
                ops[p] = pool[key][(p // 4 + shift) % len(pool[key])]
            quiet.add(len(waves))
            waves.append(ops)
    # (2) eventful neighbours: every group holds an event, the classes rotate through the positions; sub patterns across the groups
    patterns = []
    for k in kinds:
        patterns.append([k] * 16)
    if ADD in kinds:
        patterns += [[ADD, SUB] * 8, [SUB, ADD] * 8]
        prnd = random.Random(seed + 1)
        patterns += [[prnd.choice(kinds) for _ in range(16)] for _ in range(6)]
    per_kind = {k: [key for key in keys if key[1] == k] for k in kinds}
    loud_kind = {k: [key for key in per_kind[k] if key[0] in LOUD] for k in kinds}
    for pat in patterns:   # (the class under test on every other group, a carry / borrow event of any class in the groups between)
        for layout in (0, 1):
            for s in range(max(len(v) for v in per_kind.values())):
                ops = []
                for p in range(16):
                    lst = per_kind[pat[p]] if (p + layout) % 2 == 0 else loud_kind[pat[p]]
                    key = lst[(p // 2 + s) % len(lst)]
                    ops.append(pool[key][(p + s) % len(pool[key])])
                waves.append(ops)
    # (3) the limits of the operand ranges and plain random operands
    if MUL in kinds:
        big = [R, R + 1, B256 - 1, B256 - 2, 2 * R, 2 * R + 1, 5 * R, B256 - (1 << 32), 1 << 255, (1 << 255) - 1, R - 1, 1]
        bs = [R - 1, R - 2, 1, 2, (R - 1) // 2, (R + 1) // 2, rnd.randrange(R), rnd.randrange(R)]
        lim = [(a, b, MUL) for a in big for b in bs]
        while len(lim) % 16:
            lim.append((rnd.randrange(B256), rnd.randrange(R), MUL))
        waves += [lim[i:i + 16] for i in range(0, len(lim), 16)]
    for _ in range(4):
        waves.append([(lambda k: (rnd.randrange(B256 if k == MUL else R), rnd.randrange(R), k))(rnd.choice(kinds)) for _ in range(16)])
    return {"waves": waves, "quiet": quiet, "pool": pool}


def census(seq, waves, quiet):
    """Runs the waves on the emulator.  -> (results, counts, cover): per wave the 16 results; counts[(class, kind)] = group
    operations that show the class; cover[(class, kind, mode)] = set of group positions, mode "quiet" (all other groups
    of the wave's neighbourhood idle) or "loud" (both neighbours show a carry / borrow event of their own)."""
    emu = Coop4(seq)
    results, counts, cover = [], {}, {}
    for wi, ops in enumerate(waves):
        res, evs = emu.run(ops)
        results.append(res)
        loud = [bool(e & LOUD) for e in evs]
        for p, (op, ev) in enumerate(zip(ops, evs)):
            if op == IDLE[seq]:
                continue
            nb = [q for q in (p - 1, p + 1) if 0 <= q < 16]
            mode = "quiet" if wi in quiet and all(ops[q] == IDLE[seq] for q in nb) else "loud" if all(loud[q] for q in nb) else None
            for c in (ev & set(EVENTS)) | rider_classes(op, ev):
                counts[(c, op[2])] = counts.get((c, op[2]), 0) + 1
                if mode:
                    cover.setdefault((c, op[2], mode), set()).add(p)
    return results, counts, cover


# ---- one-lane sequences: vectors from the mathematics alone ----------------------------------------------------------------------
def _solve_u(u, mod, rnd, tries=400):
    t = u % mod
    for _ in range(tries):
        # (u >= a b / 2^256: a small u needs a small product, u >= mod a large one)
        a = rnd.randrange(1, B256) if u >= mod or rnd.random() < 0.5 else rnd.randrange(1, 1 << rnd.choice([1, 2, 8, 32, 64, 128, 200, 254]))
        if a % mod == 0:
            continue
        b = t * B256 * pow(a, -1, mod) % mod
        if mont_u(a, b, mod) == u:
            return a, b
    return None


def _limb_patterns(rnd, limit):
    """values below `limit` whose raw limbs are 0, 1, 2^32 - 1 in every position and in runs, the other limbs random"""
    out = []
    for v in (0, 1, M32):
        for i in range(8):
            for j in range(i, 8):
                x = rnd.randrange(B256)
                for k in range(i, j + 1):
                    x = (x & ~(M32 << (32 * k))) | (v << (32 * k))
                if x >= limit:   # keep the pattern, shrink a limb outside it (the top one if free, else give up the top of the run)
                    x &= ~(M32 << 224)
                    if j < 7:
                        x |= rnd.randrange(limit >> 224) << 224
                out.append(x)
        out.append(sum(v << (32 * k) for k in range(8)) % limit if limit < B256 else sum(v << (32 * k) for k in range(8)))
    assert all(x < limit for x in out)
    return out


@functools.lru_cache(maxsize=None)
def one_lane_mul(mod, seed=7):
    """[(a, b)]: a < 2^256, b < mod.  -> (pairs, stats) with stats naming how many pairs each class holds"""
    rnd = random.Random("mul-%d-%d" % (mod, seed))
    pairs, stats = [], {}

    def by_u(name, u, n=2):
        for _ in range(n):
            ab = _solve_u(u, mod, rnd)
            if ab is not None:
                pairs.append(ab)
                stats[name] = stats.get(name, 0) + 1
    pairs += [(0, 0), (0, mod - 1), (B256 - 1, 0), (mod, 0)]
    stats["u=0"] = 4
    for name, u in (("u=1", 1), ("u=r-1", mod - 1), ("u=r", mod), ("u=r+1", mod + 1), ("u=2r-2", 2 * mod - 2), ("u=2r-1", 2 * mod - 1)):
        by_u(name, u, 4)
    for k in range(1, 8):   # u equals the modulus in its low k words, word k differs: the subtraction's borrow runs k words or stops
        for delta in (1, -1, None):
            for _ in range(3):
                lo = mod & ((1 << (32 * k)) - 1)
                word = ((mod >> (32 * k)) & M32)
                word = (word + delta) & M32 if delta else rnd.randrange(1 << 32)
                hi = rnd.randrange(1 << (32 * (7 - k))) if k < 7 else 0
                u = lo | (word << (32 * k)) | (hi << (32 * (k + 1)))
                if u < 2 * mod - 1:
                    by_u("u=r in %d low words" % k, u, 1)
    for v in (0, M32):      # result words all zero / all ones in every position and in runs
        for i in range(8):
            for j in range(i, 8):
                t = rnd.randrange(mod)
                for k in range(i, j + 1):
                    t = (t & ~(M32 << (32 * k))) | (v << (32 * k))
                if t < mod:
                    by_u("result words %x" % v, t, 1)
                    by_u("result words %x (u >= r)" % v, t + mod, 1)
    pa, pb = _limb_patterns(rnd, B256), _limb_patterns(rnd, mod)
    for x in pa:
        pairs.append((x, rnd.randrange(mod)))
    for x in pb:
        pairs.append((rnd.randrange(B256), x))
    for x, y in zip(pa, reversed(pb)):
        pairs.append((x, y))
    stats["limb patterns"] = len(pa) + len(pb) + len(pa)
    lim = [mod, mod + 1, mod - 1, B256 - 1, B256 - 2, 2 * mod, 1, 2, B256 - (1 << 32), (1 << 255)]
    for a in lim:
        for b in (mod - 1, mod - 2, 1, rnd.randrange(mod)):
            pairs.append((a, b))
    stats["limits"] = 4 * len(lim)
    for _ in range(256):
        pairs.append((rnd.randrange(B256), rnd.randrange(mod)))
    stats["random"] = 256
    assert all(a < B256 and b < mod for a, b in pairs)
    return pairs, stats


@functools.lru_cache(maxsize=None)
def one_lane_single(mod, seed=9):
    """values below 2^256 for fr_to_mont / fr_from_mont / fr_sqr-like single-operand primitives"""
    rnd = random.Random("single-%d-%d" % (mod, seed))
    out = [0, 1, 2, mod - 1, mod, mod + 1, 2 * mod - 1, 2 * mod, B256 - 1, B256 - 2, (mod - 1) // 2, (mod + 1) // 2, 1 << 255, B256 - mod]
    out += _limb_patterns(rnd, B256)
    out += [(1 << k) for k in range(256)] + [B256 - (1 << k) for k in range(256)]
    out += [rnd.randrange(B256) for _ in range(128)]
    return out


@functools.lru_cache(maxsize=None)
def one_lane_addsub(mod, seed=11):
    """[(a, b)] with a, b < mod: a + b and a - b around 0, the modulus and the 32-bit word boundaries"""
    rnd = random.Random("addsub-%d-%d" % (mod, seed))
    pairs = []
    sums = [0, 1, 2, mod - 1, mod, mod + 1, 2 * mod - 2, 2 * mod - 3]
    for k in range(1, 8):
        for base in (0, mod):
            sums += [base + (1 << (32 * k)) + d for d in (-1, 0, 1)] + [base - (1 << (32 * k)) + d for d in (-1, 0, 1) if base]
        sums += [(mod & ((1 << (32 * k)) - 1)) | (rnd.randrange(1 << (32 * (8 - k))) << (32 * k)) for _ in range(2)]
    for s in sums:
        lo, hi = max(0, s - mod + 1), min(mod - 1, s)
        if 0 <= s and lo <= hi:
            for a in {lo, hi, rnd.randint(lo, hi), rnd.randint(lo, hi)}:
                pairs.append((a, s - a))
    diffs = [0, 1, -1, 2, -2, mod - 1, -(mod - 1)]
    for k in range(1, 8):
        diffs += [sg * ((1 << (32 * k)) + d) for sg in (1, -1) for d in (-1, 0, 1)]
    for d in diffs:
        lo, hi = max(0, -d), min(mod - 1, mod - 1 - d)   # range of b with 0 <= a = b + d < mod
        for b in {lo, hi, rnd.randint(lo, hi), rnd.randint(lo, hi)}:
            pairs.append((b + d, b))
    pat = _limb_patterns(rnd, mod)
    for x in pat:
        pairs += [(x, rnd.randrange(mod)), (rnd.randrange(mod), x), (x, x), (x, mod - x if x else 0), (x, (x + 1) % mod)]
    for _ in range(256):
        pairs.append((rnd.randrange(mod), rnd.randrange(mod)))
    assert all(0 <= a < mod and 0 <= b < mod for a, b in pairs)
    return pairs


def lane_masks(seed=13):
    """subtracting-lane masks of fr_addsub_wave: uniform, alternating, single lanes of each kind, halves, seeded random"""
    rnd = random.Random(seed)
    m = [0, M64, 0x5555555555555555, 0xaaaaaaaaaaaaaaaa, 0xffffffff, 0xffffffff00000000]
    m += [1 << i for i in (0, 1, 31, 32, 63)] + [M64 ^ (1 << i) for i in (0, 1, 31, 32, 63)]
    m += [rnd.randrange(1 << 64) for _ in range(4)]
    return m


def inv_values(seed=15):
    rnd = random.Random(seed)
    v = [0, 1, 2, 3, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2] + list(range(4, 40))
    v += [1 << k for k in range(254)] + [R - (1 << k) for k in range(254)]
    v += [rnd.randrange(R) for _ in range(300)]
    return v


# ---- the same states inside the interpreter (narrow multiplication bundles of calc_witness_batch) ---------------------------------
RINV = pow(B256, -1, R)
SHAPES = ("mul", "riders", "fused0", "fused1", "fused2", "fused3")


def interpreter_graph(builder_cls, shape, n):
    """n independent products of two inputs each (few enough to compile into one narrow bundle: class MULQ, four lanes per
    product); "riders": an addition or a subtraction of the same inputs beside every product; "fused0" .. "fused3": (x y) z + w,
    x y - w, w - x y, (x y + z) - w, chains the compiler fuses into class MULF (forced with CWC_FUSE=1001)."""
    b = builder_cls()
    xs, ys = b.input("x", n), b.input("y", n)
    fused = shape.startswith("fused")
    zs, ws = (b.input("z", n), b.input("w", n)) if fused else (None, None)
    for i in range(n):
        p = b.mul(xs[i], ys[i])
        if not fused:
            b.signal(p)
        if shape == "riders":
            b.signal(b.add(xs[i], ys[i]) if i % 2 == 0 else b.sub(xs[i], ys[i]))
        if fused:
            k = int(shape[5])
            b.signal(b.add(b.mul(p, zs[i]), ws[i]) if k == 0 else b.sub(p, ws[i]) if k == 1 else b.sub(ws[i], p) if k == 2 else b.sub(b.add(p, zs[i]), ws[i]))
    return b


@functools.lru_cache(maxsize=None)
def interpreter_rows(shape, n, n_rows=96, seed=5):
    """Input rows [1, x.., y.. (, z.., w..)]: canonical inputs x = a / 2^256 mod r, so that the Montgomery words the lanes hold
    are the operands of the vector pools.  The compiler chooses which factor of a product is passed in full: every pair of
    rows holds the same operands in both orders.  The linear operands of the fused shapes are solved so that the later stages
    land on borrow-pass events for the product's actual value."""
    rnd = random.Random("rows-%s-%d-%d" % (shape, n, seed))
    pool = build("mulr")["pool"]
    by_kind = {k: [op for (c, kk), lst in sorted(pool.items()) if kk == k for op in lst if op[0] < R] for k in (MUL, ADD, SUB)}
    tg = borrow_targets(rnd)
    names = sorted(tg)
    rows, t = [], 0
    for r in range(n_rows):
        xs, ys, zs, ws = [], [], [], []
        for i in range(n):
            # (riders: the pair makes the rider's event in one pair of rows and the product's beside it in the next)
            kind = (ADD, SUB)[i % 2] if shape == "riders" and (r // 2) % 2 == 0 else MUL
            lst = by_kind[kind]
            a, b, _ = lst[((r // 2) * n + i) % len(lst)]
            if r % 2 and not (shape == "riders" and i % 2):
                a, b = b, a
            xs.append(a * RINV % R)
            ys.append(b * RINV % R)
            if shape.startswith("fused"):
                def fit(v):
                    return v if 0 <= v < R else rnd.randrange(R)
                p = a * b * RINV % R
                k, w1, w2 = int(shape[5]), tg[names[t % len(names)]](), tg[names[(t + 3) % len(names)]]()
                t += 1
                z = rnd.randrange(R)
                if k == 0:
                    w = fit(w1 - p * z * RINV % R)
                elif k == 1:
                    w = fit(p + R - w1)
                elif k == 2:
                    w = fit(w1 - R + p)
                else:
                    z = fit(w1 - p)
                    w = fit((p + z) % R + R - w2)
                zs.append(z * RINV % R)
                ws.append(w * RINV % R)
        rows.append([1] + xs + ys + zs + ws)
    return rows


def interpreter_census(pe, blob, rows):
    """Runs the rows through tests/program_emulator.py with its observer and the observed operand words of the narrow bundles
    through the lane emulators.  -> (witnesses per row, counts of fr_vectors.EVENTS per kind, number of fused nodes seen)"""
    seen, fused = [], []
    wits = []
    for row in rows:
        got, st = pe.run(blob, row, observe=lambda name, ops: (seen if name == "MULQ" else fused).append(ops))
        assert st == 0
        wits.append(got)
    ops = [(a, b, sub) for a, b, sub in seen]
    lin_ops = []
    for a, b, op2, x2, op3, x3 in fused:   # the stages of a fused node, each as the lanes compute it
        ops.append((a, b, MUL))
        acc = a * b * RINV % R
        for code, x in ((op2, x2), (op3, x3)):
            if code == 1:
                ops.append((x, acc, MUL))
                acc = acc * x * RINV % R
            elif code:
                o = (acc, x, ADD) if code == 2 else (acc, x, SUB) if code == 3 else (x, acc, SUB)
                lin_ops.append(o)
                acc = want(*o)
    counts = {}
    for seq, lst in (("mulr", ops), ("lin", lin_ops)):
        emu = Coop4(seq)
        for i in range(0, len(lst), 16):
            chunk = lst[i:i + 16]
            res, evs = emu.run(chunk + [IDLE[seq]] * (16 - len(chunk)))
            for op, got, ev in zip(chunk, res, evs):
                assert got == want(*op)
                for c in ev & set(EVENTS):
                    counts[(c, op[2])] = counts.get((c, op[2]), 0) + 1
    return wits, counts, len(fused)
