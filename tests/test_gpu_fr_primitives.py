"""The device field primitives on a real MI355X at the carry and borrow events of tests/fr_vectors.py.

tests/native/fr_primitives.hip (compiled here) runs every primitive of csrc/fr_gfx950.hpp and r1cs/fq_gfx950.hpp as the product
calls it, in full 64-lane waves over several workgroups, on operand records this file writes, and returns raw limbs.  The
reference is Python big integers; every comparison is exact.  One process under one time limit per family of primitives; after a
process that did not exit with status 0 no further family is started.

Left out: fr_mul_coop2 / fr_mul_coop8 (used by the micro-benchmark tools/ubench/coop_mul.hip only; the emulator-observed vector
builder is written for the K = 4 lane layout)."""
import os
import random
import subprocess

import numpy as np
import pytest

import fr_vectors as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, Q, B256, M32, M64 = V.R, V.Q, V.B256, V.M32, V.M64
OP = dict(FR_MUL=1, FR_MUL_WAVE=2, FR_SQR=3, FR_TO_MONT=4, FR_FROM_MONT=5, FR_ADD=6, FR_SUB=7, FR_ADD_WAVE=8, FR_SUB_WAVE=9,
          FR_ADDSUB_WAVE=10, FR_NEG=11, FR_MUL_CHAIN=12, FR_MUL_WAVE_CHAIN=13,
          FQ_MUL=20, FQ_ADD=21, FQ_SUB=22, FQ_NEG=23, FQ_TO_MONT=24, FQ_FROM_MONT=25, FQ_MUL_CHAIN=26, FR_INV=30,
          DIV_DIGITS=40, DIV_SHORT=41, DIV_2BY1=42, DIV_RECIP=43, DIV_3BY2=44, DIV_128=45,
          COOP4=50, COOP4R=51, ADDSUB_COOP4=52, COOP4_CHAIN=53, COOP4_FUSED_CHAIN=54)
_state = {"failed": None}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fr_primitives") / "fr_primitives"
    csrc = os.path.join(ROOT, "circom-witnesscalc_amd")
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(csrc, "csrc"), "-I" + os.path.join(csrc, "r1cs"),
                    os.path.join(ROOT, "tests", "native", "fr_primitives.hip"), "-o", str(exe)], check=True, timeout=1800)
    return str(exe)


def words(values, n_words):
    """ints -> u32 array [len, n_words], little-endian limbs"""
    buf = b"".join(int(v).to_bytes(4 * n_words, "little") for v in values)
    return np.frombuffer(buf, dtype="<u4").reshape(len(values), n_words)


def ints(arr, n_words=8):
    """u32 array [n, k * n_words] -> list of n lists of k ints"""
    arr = np.ascontiguousarray(arr.astype("<u4"))
    n, w = arr.shape
    raw = arr.tobytes()
    step = 4 * n_words
    return [[int.from_bytes(raw[(i * w * 4) + j * step:(i * w * 4) + (j + 1) * step], "little") for j in range(w // n_words)] for i in range(n)]


def run_family(exe, tmp_path, name, sections, timeout=240):
    """sections: [(op, records u32 [n, iw], out_words, param)] -> [u32 [n, ow]] (padding rows are the caller's)"""
    if _state["failed"]:
        pytest.fail("not started: the harness process of family %r did not exit cleanly" % _state["failed"])
    fin, fout = tmp_path / (name + ".in"), tmp_path / (name + ".out")
    with open(fin, "wb") as f:
        for op, rec, ow, param in sections:
            rec = np.ascontiguousarray(rec, dtype="<u4")
            f.write(np.array([op, rec.shape[0], rec.shape[1], ow, param], dtype="<u4").tobytes())
            f.write(rec.tobytes())
    p = subprocess.run(["timeout", "-k", "10", str(timeout), exe, str(fin), str(fout)], capture_output=True, text=True)
    if p.returncode != 0:
        _state["failed"] = name
        pytest.fail("harness family %r: exit status %d\n%s\n%s" % (name, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
    raw = np.fromfile(fout, dtype="<u4")
    out, pos = [], 0
    for op, rec, ow, param in sections:
        n = rec.shape[0]
        out.append(raw[pos:pos + n * ow].reshape(n, ow))
        pos += n * ow
    assert pos == raw.size
    return out


def pad(rows, filler, mult=64):
    rows = list(rows)
    n = len(rows)
    while len(rows) % mult:
        rows.append(filler)
    return rows, n


def pair_rec(pairs, filler=(0, 0)):
    rows, n = pad(pairs, filler)
    return np.concatenate([words([a for a, _ in rows], 8), words([b for _, b in rows], 8)], axis=1), n


def one_rec(vals):
    rows, n = pad(vals, 0)
    return words(rows, 8), n


def mont(a, b, mod):
    return a * b * pow(B256, -1, mod) % mod


def check(name, got_arr, n, inputs, wantf):
    got = ints(got_arr[:n])
    bad = [(i, inputs[i], g) for i, g in enumerate(got) if g != wantf(inputs[i])]
    assert not bad, "%s: %d of %d wrong; first: input %s got %s want %s" % (
        name, len(bad), n, [hex(x) if isinstance(x, int) else x for x in (bad[0][1] if isinstance(bad[0][1], tuple) else (bad[0][1],))],
        [hex(x) for x in bad[0][2]], [hex(x) for x in wantf(bad[0][1])])


def chain_want(a, b, mod, steps=64):
    out = []
    for i in range(steps):
        b = mont(a, b, mod)
        if i < 8:
            out.append(b)
    return out + [b]


def _mul_family(harness, tmp_path, mod, prefix, ops):
    pairs, _ = V.one_lane_mul(mod)
    rec, n = pair_rec(pairs)
    sq = [x for x in V.one_lane_single(mod) if x < mod] + [a for a, _ in pairs if a < mod][:256]
    sq_rec, n_sq = one_rec(sq)
    single = V.one_lane_single(mod)
    s_rec, n_s = one_rec(single)
    rnd = random.Random(5)
    chain = pairs[::7][:192] + [(rnd.randrange(B256), rnd.randrange(mod)) for _ in range(64)]
    c_rec, n_c = pair_rec(chain)
    sections, checks = [], []
    for opname in ops["mul"]:
        sections.append((OP[opname], rec, 8, 0))
        checks.append((opname, n, pairs, lambda p: [mont(p[0], p[1], mod)]))
    for opname in ops["sqr"]:
        sections.append((OP[opname], sq_rec, 8, 0))
        checks.append((opname, n_sq, sq, lambda x: [mont(x, x, mod)]))
    sections.append((OP[prefix + "_TO_MONT"], s_rec, 8, 0))
    checks.append((prefix + "_TO_MONT", n_s, single, lambda x: [x * B256 % mod]))
    sections.append((OP[prefix + "_FROM_MONT"], s_rec, 8, 0))
    checks.append((prefix + "_FROM_MONT", n_s, single, lambda x: [x * pow(B256, -1, mod) % mod]))
    for opname in ops["chain"]:
        sections.append((OP[opname], c_rec, 72, 64))
        checks.append((opname, n_c, chain, lambda p: chain_want(p[0], p[1], mod)))
    outs = run_family(harness, tmp_path, prefix.lower() + "_mul", sections)
    for (opname, n_, inputs, wantf), got in zip(checks, outs):
        check(opname, got, n_, inputs, wantf)


def test_fr_one_lane_montgomery(harness, tmp_path):
    """fr_mul, fr_mul_wave, fr_sqr, fr_to_mont, fr_from_mont on the vectors chosen by u (fr_vectors.one_lane_mul) and b <- a b
    chains of 64 (compared at each of the first eight steps and at the end)"""
    _mul_family(harness, tmp_path, R, "FR", {"mul": ["FR_MUL", "FR_MUL_WAVE"], "sqr": ["FR_SQR"], "chain": ["FR_MUL_CHAIN", "FR_MUL_WAVE_CHAIN"]})


def test_fq_one_lane(harness, tmp_path):
    _mul_family(harness, tmp_path, Q, "FQ", {"mul": ["FQ_MUL"], "sqr": [], "chain": ["FQ_MUL_CHAIN"]})
    pairs = V.one_lane_addsub(Q)
    rec, n = pair_rec(pairs)
    neg = sorted({a for a, _ in pairs} | {0, 1, Q - 1})
    n_rec, n_n = one_rec(neg)
    outs = run_family(harness, tmp_path, "fq_lin", [(OP["FQ_ADD"], rec, 8, 0), (OP["FQ_SUB"], rec, 8, 0), (OP["FQ_NEG"], n_rec, 8, 0)])
    check("FQ_ADD", outs[0], n, pairs, lambda p: [(p[0] + p[1]) % Q])
    check("FQ_SUB", outs[1], n, pairs, lambda p: [(p[0] - p[1]) % Q])
    check("FQ_NEG", outs[2], n_n, neg, lambda x: [(Q - x) % Q])


def test_fr_add_sub(harness, tmp_path):
    """fr_add, fr_sub, their interleaved _wave forms, fr_neg, and fr_addsub_wave under every lane mask of fr_vectors.lane_masks"""
    pairs = V.one_lane_addsub(R)
    rec, n = pair_rec(pairs)
    neg = sorted({a for a, _ in pairs} | {0, 1, R - 1})
    n_rec, n_n = one_rec(neg)
    sections = [(OP[o], rec, 8, 0) for o in ("FR_ADD", "FR_SUB", "FR_ADD_WAVE", "FR_SUB_WAVE")] + [(OP["FR_NEG"], n_rec, 8, 0)]
    masks = V.lane_masks()
    lanes = np.arange(rec.shape[0]) % 64
    for m in masks:
        flag = np.array([(m >> int(l)) & 1 for l in lanes], dtype="<u4").reshape(-1, 1)
        sections.append((OP["FR_ADDSUB_WAVE"], np.concatenate([rec, flag], axis=1), 8, 0))
    outs = run_family(harness, tmp_path, "fr_lin", sections)
    check("FR_ADD", outs[0], n, pairs, lambda p: [(p[0] + p[1]) % R])
    check("FR_SUB", outs[1], n, pairs, lambda p: [(p[0] - p[1]) % R])
    check("FR_ADD_WAVE", outs[2], n, pairs, lambda p: [(p[0] + p[1]) % R])
    check("FR_SUB_WAVE", outs[3], n, pairs, lambda p: [(p[0] - p[1]) % R])
    check("FR_NEG", outs[4], n_n, neg, lambda x: [(R - x) % R])
    for m, got in zip(masks, outs[5:]):
        idx = list(range(n))
        check("FR_ADDSUB_WAVE mask %x" % m, got, n, idx, lambda i: [(pairs[i][0] - pairs[i][1]) % R if (m >> (i % 64)) & 1 else (pairs[i][0] + pairs[i][1]) % R])


def test_fr_inv_device_body(harness, tmp_path):
    """fr_inv as the device compiles it (the asm matrix update of safegcd), Montgomery in and out, against pow(x, -1, r): the
    listed values both as the field element and as the raw pattern the divsteps see"""
    vals = V.inv_values()
    ins_ = sorted(set(vals) | {v * B256 % R for v in vals})
    rec, n = one_rec(ins_)
    (got,) = run_family(harness, tmp_path, "fr_inv", [(OP["FR_INV"], rec, 8, 0)])
    check("FR_INV", got, n, ins_, lambda y: [pow(y, -1, R) * B256 * B256 % R if y else 0])


def _div_operands(rnd):
    def bits(n):
        return (rnd.getrandbits(n) | (1 << (n - 1))) if n > 0 else 0
    ab = []
    for it in range(6000):
        a, b = bits(rnd.randrange(257)), bits(1 + rnd.randrange(256))
        if it % 7 == 0:
            b = sum((rnd.choice([M32, 0]) if rnd.random() < 0.5 else rnd.getrandbits(32)) << (32 * i) for i in range(8)) or 1
        if it % 11 == 0:
            a = b ^ rnd.randrange(2)
        if it % 13 == 0:
            a = B256 - 1
        if it % 17 == 0:
            b = 1 << rnd.randrange(256)
        if it % 19 == 0:
            b = (0x80000000 << 224) | (rnd.getrandbits(32) << (32 * rnd.randrange(7)))
        if it % 23 == 0:   # the divisor's leading 32 bits are 0x80000000 / 0xffffffff at any length
            n = rnd.randrange(32, 257)
            b = (rnd.choice([0x80000000, M32]) << (n - 32)) | rnd.getrandbits(n - 32) if n > 32 else rnd.choice([0x80000000, M32])
        if it % 29 == 0:   # numerators whose top words equal the divisor's: the estimate is capped at 2^32 - 1
            j = rnd.randrange(8)
            a = ((b << (32 * j)) + rnd.choice([-1, 0, 1, rnd.getrandbits(32 * j) if j else 0, -rnd.getrandbits(32)])) % B256
        if it % 31 == 0:
            nb = b.bit_length()
            a = ((b >> max(0, nb - 64)) << rnd.randrange(0, 193)) | rnd.getrandbits(64)
        ab.append((a % B256, b % B256 or 1))
    return ab


def test_divisions_device(harness, tmp_path):
    """u256_divrem_digits (digits / bitlen_b derived wave-wide as the Idiv / Mod bundles do), u128_divrem_64, u256_divrem_128 and the
    reciprocal divisions against divmod, on the edge classes of tests/native/div_*_test.cc plus divisors whose leading word is
    0x80000000 / 0xffffffff and numerators that start with the divisor's leading words"""
    rnd = random.Random(41)
    ab = _div_operands(rnd)
    d_rec, n_d = pair_rec(ab, (0, 1))
    short = [(a % (1 << 128), (b % (1 << 64)) or 1) for a, b in ab]
    short += [((b << 64 | rnd.getrandbits(64)) % (1 << 128), b) for _, b in short[:500]]
    s_rec, n_s = pair_rec(short, (0, 1))

    def pick():
        k = rnd.randrange(8)
        return [0, M64, 1 << rnd.randrange(64), (1 << rnd.randrange(64)) - 1, rnd.getrandbits(64) >> rnd.randrange(64)][k] if k < 5 else rnd.getrandbits(64)

    def norm():
        k = rnd.randrange(8)
        return [1 << 63, M64, (1 << 63) + rnd.randrange(1000), M64 - rnd.randrange(1000), (1 << 63) | (1 << rnd.randrange(63)),
                (1 << 63) | ((1 << rnd.randrange(63)) - 1), (0x80000000 << 32) | rnd.getrandbits(32), (M32 << 32) | rnd.getrandbits(32)][k] if rnd.random() < 0.5 else rnd.getrandbits(64) | (1 << 63)
    two = []
    for it in range(6000):
        dn = norm()
        u1 = rnd.choice([0, dn - 1, pick() % dn, rnd.randrange(dn)])
        two.append((u1, rnd.choice([pick(), M64, 0]), dn))
    rows, n_2 = pad(two, (0, 0, 1 << 63))
    t_rec = np.concatenate([words([r[i] for r in rows], 2) for i in range(3)], axis=1)
    rec4 = []
    for it in range(6000):
        d = pick() or 1 + rnd.randrange(3)
        th, tl = pick(), pick()
        if it % 3 == 0:
            th %= d
        if it % 5 == 0:
            th = d - 1
        if it % 7 == 0:
            th, tl = d, 0
        if it % 11 == 0:
            th, tl = d - 1, M64
        rec4.append((th, tl, d, 1 if th >= d else rnd.randrange(2)))
    rows, n_4 = pad(rec4, (0, 0, 1, 0))
    r_rec = np.concatenate([words([r[i] for r in rows], 2) for i in range(3)] + [words([r[3] for r in rows], 1)], axis=1)
    three = []
    for it in range(6000):
        d1, d0 = norm(), pick()
        d = (d1 << 64) | d0
        hi = rnd.choice([0, d - 1, rnd.randrange(d), (pick() << 64 | pick()) % d, d - 1 - rnd.randrange(4) if d > 4 else 0])
        three.append((hi >> 64, hi & M64, rnd.choice([pick(), M64, 0, d0, (d0 - 1) & M64]), d1, d0))
    rows, n_3 = pad(three, (0, 0, 0, 1 << 63, 0))
    h_rec = np.concatenate([words([r[i] for r in rows], 2) for i in range(5)], axis=1)
    wide = []
    for it in range(4000):
        bh, bl = pick() or 1 + rnd.randrange(5), pick()
        if it % 9 == 0:
            bh, bl = 1, 0
        if it % 11 == 0:
            bh, bl = M64, M64
        if it % 13 == 0:
            bh = 1 << 56
        b = (bh << 64) | bl
        a = sum(pick() << (64 * i) for i in range(4))
        if it % 4 == 0:
            a %= 1 << 242
        if it % 5 == 0:
            a %= 1 << 128
        if it % 7 == 0:
            a = b
        if it % 17 == 0:
            a = b - 1
        if it % 19 == 0:
            a = B256 - 1
        wide.append((a, b))
    w_rec, n_w = pair_rec(wide, (0, 1 << 64))
    outs = run_family(harness, tmp_path, "div", [(OP["DIV_DIGITS"], d_rec, 16, 0), (OP["DIV_SHORT"], s_rec, 16, 0), (OP["DIV_2BY1"], t_rec, 6, 0),
                                                 (OP["DIV_RECIP"], r_rec, 6, 0), (OP["DIV_3BY2"], h_rec, 8, 0), (OP["DIV_128"], w_rec, 16, 0)])
    check("u256_divrem_digits", outs[0], n_d, ab, lambda p: list(divmod(p[0], p[1])))
    check("u128_divrem_64", outs[1], n_s, short, lambda p: list(divmod(p[0], p[1])))
    got = ints(outs[2][:n_2], 2)
    for (u1, u0, dn), g in zip(two, got):
        assert g == list(divmod((u1 << 64) | u0, dn)) + [((1 << 128) - 1) // dn - (1 << 64)], ("div2by1", hex(u1), hex(u0), hex(dn), g)
    got = ints(outs[3][:n_4], 2)
    for (th, tl, d, high), g in zip(rec4, got):
        q, rem = divmod((th << 64) | tl, d)
        assert g == [q >> 64, q & M64, rem], ("u128_divrem_64_recip", hex(th), hex(tl), hex(d), high, g)
    got = ints(outs[4][:n_3], 2)
    for (u2, u1, u0, d1, d0), g in zip(three, got):
        d = (d1 << 64) | d0
        q, rem = divmod((u2 << 128) | (u1 << 64) | u0, d)
        assert g == [q, rem >> 64, rem & M64, ((1 << 192) - 1) // d - (1 << 64)], ("div3by2", hex(u2), hex(u1), hex(u0), hex(d1), hex(d0), g)
    check("u256_divrem_128", outs[5], n_w, wide, lambda p: list(divmod(p[0], p[1])))


def _coop_rec(ops, with_kind):
    cols = [words([o[0] for o in ops], 8), words([o[1] for o in ops], 8)]
    if with_kind:
        cols.append(words([o[2] for o in ops], 1))
    return np.concatenate(cols, axis=1)


def test_cooperative_sequences_at_the_events(harness, tmp_path):
    """fr_mul_coop4, fr_mul_coop4r, fr_addsub_coop4 in the interpreter's lane layout on the waves of fr_vectors.build: the states the
    emulator counted in tests/test_fr_primitives_host.py (P with carry-in / borrow-in, two adjacent propagating lanes, SEL decided
    through a propagating lane, the rider edges), in every group position, beside idle and eventful groups"""
    sections, flat = [], []
    for seq, opname in (("mul", "COOP4"), ("mulr", "COOP4R"), ("lin", "ADDSUB_COOP4")):
        ops = [op for wave in V.build(seq)["waves"] for op in wave]
        assert len(ops) % 16 == 0
        while len(ops) % 64:   # (whole workgroups of four waves are not required; whole waves are: 16 groups)
            ops.append(V.IDLE[seq])
        flat.append(ops)
        sections.append((OP[opname], _coop_rec(ops, seq != "mul"), 8, 0))
    outs = run_family(harness, tmp_path, "coop", sections)
    for (seq, ops, got) in zip(("mul", "mulr", "lin"), flat, outs):
        check("coop4 " + seq, got, len(ops), ops, lambda o: [V.want(*o)])


def test_cooperative_chains(harness, tmp_path):
    """Back-to-back cooperative blocks meet each other's wait states: b <- a b 64 times, and the fused narrow bundle's pattern
    (product, product by the running value, then fr_addsub_coop4 with add, subtract, reversed subtract) 13 rounds = 65 blocks;
    compared at every step of the first eight (ten for the fused pattern) and at the end.  The linear operands of the first
    round are solved so that its three additions / subtractions land on borrow-pass events as well."""
    rnd = random.Random(77)
    mul_ops = [op for wave in V.build("mul")["waves"] for op in wave if op != V.IDLE["mul"]]
    chain = [(a, b) for a, b, _ in mul_ops[::3]][:240]
    chain += [(rnd.randrange(B256), rnd.randrange(R)) for _ in range(16)]
    while len(chain) % 16:
        chain.append((0, 0))
    tg = V.borrow_targets(rnd)
    names = sorted(tg)
    fused = []
    for i, (a, b) in enumerate(chain):
        x2 = rnd.choice([rnd.randrange(R), rnd.randrange(B256), R - 1, 1])
        acc = mont(x2, mont(a, b, R), R)

        def fit(x):
            return x if 0 <= x < R else rnd.randrange(R)
        x3 = fit(tg[names[i % len(names)]]() - acc)
        acc3 = (acc + x3) % R
        x4 = fit(acc3 + R - tg[names[(i + 1) % len(names)]]())
        acc4 = (acc3 - x4) % R
        x5 = fit(tg[names[(i + 2) % len(names)]]() - R + acc4)
        fused.append((a, b, x2, x3, x4, x5))
    c_rec = np.concatenate([words([c[i] for c in chain], 8) for i in range(2)], axis=1)
    f_rec = np.concatenate([words([c[i] for c in fused], 8) for i in range(6)], axis=1)
    outs = run_family(harness, tmp_path, "coop_chain", [(OP["COOP4_CHAIN"], c_rec, 72, 64), (OP["COOP4_FUSED_CHAIN"], f_rec, 88, 13)])
    check("coop4 chain", outs[0], len(chain), chain, lambda p: chain_want(p[0], p[1], R))

    def fused_want(rec):
        a, acc, x2, x3, x4, x5 = rec
        steps = []
        for _ in range(13):
            acc = mont(a, acc, R); steps.append(acc)
            acc = mont(x2, acc, R); steps.append(acc)
            acc = (acc + x3) % R; steps.append(acc)
            acc = (acc - x4) % R; steps.append(acc)
            acc = (x5 - acc) % R; steps.append(acc)
        return steps[:10] + [acc]
    check("coop4 fused chain", outs[1], len(fused), fused, fused_want)


def test_events_inside_the_interpreter(pkg, monkeypatch):
    """The cooperative vectors through calc_witness_batch: graphs of a few independent products (alone, with additions and
    subtractions at the same level, and as fused chains), inputs x = a / 2^256 mod r in both operand orders, at tile keys 1, 2, 4,
    2 | divider and 2 | divider | two streams (eight-wave workgroups forced).  Every program is checked to hold narrow bundles
    (tests/test_fr_primitives_host.py shows which events their operands reach); reference: the C oracle for every row, plain
    Python for a sample."""
    from oracle import cbind, model
    import test_fr_primitives_host as H
    monkeypatch.setenv("CWC_FUSE", "1001")
    monkeypatch.setenv("CWC_STREAM_TILES_PER_WORKGROUP", "2")
    ran = 0
    for shape, n in H.INTERPRETER_CASES:
        for key in H.INTERPRETER_KEYS:
            case = H.interpreter_case(pkg, shape, n, key)
            if case is None:
                continue
            data, rows, blob, need = case
            nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
            inp = cbind.ints_to_array(rows)
            want, wst = cbind.Graph(data).evaluate_batch(inp)
            assert not wst.any()
            g = pkg.Graph(data)
            g.set_tile_width(key)
            got, st = g.calc_witness_batch(inp)
            assert not st.any() and np.array_equal(got, want), (shape, n, hex(key))
            for i in range(0, len(rows), 7):
                assert cbind.array_to_ints(got[i]) == model.evaluate(nodes, rows[i], wit), (shape, n, hex(key), i)
            ran += 1
    assert ran >= 30
