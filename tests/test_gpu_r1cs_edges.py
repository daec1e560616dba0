"""The R1CS check kernel (r1cs/check.hip) at its edges, on an MI355X: synthetic constraint systems that every completed row
satisfies by construction (tests/r1cs_fixtures.planted_system), compared exactly with the big-integer checker.

What each test reaches: coefficients that coincide with 0, +-1 and the Montgomery constants, mixed factor kinds and
duplicate wires; combination lengths around the 4-way unroll; failing constraints whose file order and device (length
bucketed) order disagree; rows holding values at or above r; padded rows and constraints at every tile width; and the
host, device, .wtns and CLI entry points on the same rows."""
import os
import random
import subprocess

import numpy as np
import pytest

import cwc_import
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
SAT = 0xFFFFFFFF
R = F.R
TILE_WIDTHS = (1, 2, 4, 8, 16, 32, 64, 0)
EDGE_POOL = [0, 1, R - 1, 2, R - 2, (R + 1) // 2, F.MONT_R, F.MONT_R_INV, F.MONT_R2, (1 << 255) % R, None]
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 600, 2500)

pytestmark = pytest.mark.gpu


def _r1cs(n_wires, constraints):
    return PKG.R1cs(F.write_r1cs(n_wires, constraints))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _device(r, arr, montgomery=False):
    import torch
    d = torch.from_numpy(arr).cuda()
    first, nfail = r.check_batch_device(d, montgomery=montgomery)
    torch.cuda.synchronize()
    return _u32(first), _u32(nfail)


def _mont_rows(rows):
    return [[F.to_montgomery(x) for x in row] for row in rows]


def _expect(constraints, rows, tampered):
    """per-row (first, n): the checker on the tampered rows, (SAT, 0) on the others (planted rows)"""
    first = np.full(len(rows), SAT, dtype=np.uint32)
    nfail = np.zeros(len(rows), dtype=np.uint32)
    for s in tampered:
        first[s], nfail[s] = F.check(constraints, [x % R for x in rows[s]])
    return first, nfail


def _assert_paths(r, rows, want, paths=("host", "device", "montgomery"), widths=TILE_WIDTHS, what=""):
    """every requested entry point at every tile width gives exactly `want` ((first, n) arrays)"""
    canon = F.rows_array(rows)
    mont = F.rows_array(_mont_rows(rows)) if "montgomery" in paths else None
    for t in widths:
        r.set_tile_width(t)
        for p in paths:
            if p == "host":
                got = r.check_batch(canon)
            elif p == "device":
                got = _device(r, canon)
            else:
                got = _device(r, mont, montgomery=True)
            for k, name in ((0, "first_failed"), (1, "n_failed")):
                bad = np.flatnonzero(got[k] != want[k])
                assert bad.size == 0, "%s: %s at tile width %d, path %s: rows %s got %s want %s" % (
                    what, name, t, p, bad[:8].tolist(), got[k][bad[:8]].tolist(), want[k][bad[:8]].tolist())
    r.set_tile_width(0)


def _tamper(rnd, row, wires):
    for w in wires:
        row[w] = (row[w] + rnd.randrange(1, R)) % R


# -- 1. coefficient and factor-kind edges ------------------------------------------------------------------------------------
def test_coefficient_and_kind_edges(pkg):
    rnd = random.Random(101)
    small = (0, 1, 2, 3, 4, 5, 6, 9)
    shapes = [dict(a=rnd.choice(small), b=rnd.choice(small), c=rnd.choice(small), dup=True, edge=True) for _ in range(300)]
    shapes += [dict(a=3, b=2, c=0, out=False), dict(a=0, b=0, c=0, out=False)]
    P = F.planted_system(rnd, 24, shapes, EDGE_POOL)
    cons = P.constraints
    coefs = [c for con in cons for lc in con for _, c in lc]
    for v in EDGE_POOL[:-1]:
        assert v in coefs, v
    # a cancelling +1 / -1 pair on one wire somewhere
    assert any(any((w, 1) in lc and (w, R - 1) in lc for w, _ in lc) for con in cons for lc in con)
    r = _r1cs(P.n_wires, cons)
    assert r.info["n_factors_a"] == sum(len(a) for a, _, _ in cons)
    rows = [P.complete(rnd) for _ in range(37)]
    assert F.check(cons, rows[0]) == (SAT, 0)
    tampered = [3, 20, 36]
    for s in tampered:
        _tamper(rnd, rows[s], rnd.sample(range(1, P.n_wires), 3))
    want = _expect(cons, rows, tampered)
    assert all(want[1][s] >= 1 for s in tampered)
    _assert_paths(r, rows, want, what="edge pool")


def test_many_distinct_coefficients(pkg):
    """more distinct general coefficients than 16 bits index"""
    rnd = random.Random(102)
    shapes = [dict(a=14, b=14, c=14) for _ in range(1800)]
    P = F.planted_system(rnd, 40, shapes, [None])
    cons = P.constraints
    assert len({c for con in cons for lc in con for _, c in lc} - {1, R - 1}) >= 70000
    r = _r1cs(P.n_wires, cons)
    rows = [P.complete(rnd) for _ in range(9)]
    tampered = [4, 8]
    for s in tampered:
        _tamper(rnd, rows[s], [rnd.choice(P.free)])
    want = _expect(cons, rows, tampered)
    assert all(want[1][s] >= 1 for s in tampered)
    _assert_paths(r, rows, want, what="70k coefficients")


# -- 2. combination lengths ------------------------------------------------------------------------------------------------
def test_combination_lengths(pkg):
    rnd = random.Random(103)
    pool = [1, R - 1, 2, None]
    shapes = []
    for n in LENGTHS:
        m = rnd.choice((1, 2, 3, 5))
        shapes += [dict(a=n, b=m, c=rnd.choice(LENGTHS[:9]), dup=True), dict(a=m, b=n, c=m), dict(a=m, b=m, c=n, dup=True),
                   dict(a=0, b=n, c=m), dict(a=n, b=0, c=m),                    # one factor side empty: A B = 0
                   dict(a=n, b=m, c=0, out=False), dict(a=0, b=n, c=0, out=False)]  # C empty
    shapes.append(dict(a=0, b=0, c=0, out=False))
    rnd.shuffle(shapes)
    P = F.planted_system(rnd, 30, shapes, pool)
    # near misses: a copy of a satisfied constraint with C's constant term off by one fails in every row
    picks = set(rnd.sample(range(len(P.constraints)), 6))
    cons, near = [], []
    for j, (a, b, c) in enumerate(P.constraints):
        cons.append((a, b, c))
        if j in picks:
            near.append(len(cons))
            cons.append((a, b, c + [(0, rnd.choice((1, R - 1)))]))
    r = _r1cs(P.n_wires, cons)
    rows = [P.complete(rnd) for _ in range(11)]
    for row in rows[:2]:
        assert F.check(P.constraints, row) == (SAT, 0)
    tampered = [5, 10]
    for s in tampered:
        _tamper(rnd, rows[s], rnd.sample(P.free, 2))
    first, nfail = _expect(cons, rows, tampered)
    for s in range(len(rows)):
        if s not in tampered:
            first[s], nfail[s] = min(near), len(near)
    assert F.check(cons, rows[0]) == (min(near), len(near))
    _assert_paths(r, rows, (first, nfail), what="lengths")


# -- 3. file order against device order ---------------------------------------------------------------------------------------
def test_first_failed_is_the_file_index(pkg):
    """Long constraints first in the file, short ones after: the loader's length buckets put the short ones first on the
    device, so a device index is never the file index a row must report."""
    rnd = random.Random(104)
    shapes = [dict(a=rnd.randrange(30, 90), b=rnd.randrange(20, 60), c=rnd.randrange(10, 40)) for _ in range(24)]
    shapes += [dict(a=1, b=1, c=rnd.choice((0, 1))) for _ in range(300)]
    P = F.planted_system(rnd, 16, shapes, [1, R - 1, None])
    cons = P.constraints
    r = _r1cs(P.n_wires, cons)
    out_of = {j: 1 + j for j in range(len(cons))}  # every shape owns an output wire, in order
    rows = [P.complete(rnd) for _ in range(70)]
    cases = {
        2: [out_of[5], out_of[len(cons) - 1]],                 # a long and a short one
        9: [out_of[len(cons) - 1]],                            # a short one only
        31: [out_of[23]],                                      # a long one only
        40: [out_of[j] for j in (30, 77, 150, 200, 260, 311)],  # six short ones
        63: [out_of[0], out_of[100], out_of[250]],
        69: rnd.sample(P.free, 2),
    }
    for s, wires in cases.items():
        _tamper(rnd, rows[s], wires)
    want = _expect(cons, rows, sorted(cases))
    assert want[0][2] == 5 and want[1][2] >= 2 and want[0][9] == len(cons) - 1 and want[1][40] >= 5
    _assert_paths(r, rows, want, paths=("host", "device"), what="file order")


# -- 4. rows holding values at or above r ----------------------------------------------------------------------------------
def _lift(rnd, x):
    """x + k r for a random k in 1..4 that keeps the value below 2^256"""
    kmax = min(4, ((1 << 256) - 1 - x) // R)
    return x + rnd.randint(1, kmax) * R


def test_rows_above_r(pkg):
    rnd = random.Random(105)
    small = (1, 2, 3, 4, 5, 7)
    shapes = [dict(a=rnd.choice(small), b=rnd.choice(small), c=rnd.choice(small), dup=True, edge=True) for _ in range(120)]
    P = F.planted_system(rnd, 12, shapes, [1, R - 1, None, 2])
    cons = P.constraints
    r = _r1cs(P.n_wires, cons)
    top = (1 << 256) - 1
    f_top = P.free[-1]  # the last wire: in every side of length >= 2
    rows = [P.complete(rnd, fixed={f_top: top % R}) for _ in range(20)]
    mont = _mont_rows(rows)
    lifted = [[_lift(rnd, x) for x in row] for row in rows]
    lifted_m = [[_lift(rnd, x) for x in row] for row in mont]
    for row, row_m in zip(lifted, lifted_m):
        assert all(x >= R for x in row) and all(x >= R for x in row_m)
    for row in lifted[::2]:  # 2^256 - 1 itself, where it is congruent to the planted value
        row[f_top] = top
    tampered = [7, 19]
    for s in tampered:
        w = rnd.choice(P.free[:-1])
        d = rnd.randrange(1, R)
        lifted[s][w] = (lifted[s][w] % R + d) % R + R  # still above r, no longer the planted value
        lifted_m[s][w] = (lifted_m[s][w] % R + F.to_montgomery(d)) % R + R
    want = _expect(cons, lifted, tampered)
    assert all(want[1][s] >= 1 for s in tampered)
    canon, mont_arr = F.rows_array(lifted), F.rows_array(lifted_m)
    for t in TILE_WIDTHS:
        r.set_tile_width(t)
        for name, got in (("host", r.check_batch(canon)), ("device", _device(r, canon)),
                          ("montgomery", _device(r, mont_arr, montgomery=True))):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (t, name, got, want)


# -- 5. padded rows and constraints, striding ------------------------------------------------------------------------------
def test_padding_at_every_tile_width(pkg):
    """The failing row is the last one and the failing constraint the last one: a padded lane (a duplicate of the last row)
    or a padded constraint slot (a duplicate of the last constraint) that reported would inflate n_failed."""
    rnd = random.Random(106)
    P = F.planted_system(rnd, 8, [dict(a=rnd.randint(1, 3), b=rnd.randint(1, 3), c=rnd.randint(0, 2)) for _ in range(65)], [1, None])
    base = [P.complete(rnd) for _ in range(131)]
    systems = {}
    for t in (1, 2, 4, 8, 16, 32, 64):
        g = 64 // t
        for nc in sorted({1, g - 1, g, g + 1} - {0}):
            if nc not in systems:
                systems[nc] = _r1cs(P.n_wires, P.constraints[:nc])
            r = systems[nc]
            r.set_tile_width(t)
            for batch in sorted({1, t - 1, t, t + 1, 2 * t + 3} - {0}):
                rows = [list(x) for x in base[:batch]]
                _tamper(rnd, rows[-1], [1 + nc - 1])  # constraint nc - 1's output: read by no other of the first nc
                first, nfail = np.full(batch, SAT, dtype=np.uint32), np.zeros(batch, dtype=np.uint32)
                first[-1], nfail[-1] = nc - 1, 1
                got = _device(r, F.rows_array(rows))
                assert np.array_equal(got[0], first) and np.array_equal(got[1], nfail), (t, nc, batch, got)
    # the tile width forced above the batch
    r = systems[1]
    r.set_tile_width(64)
    rows = [list(x) for x in base[:3]]
    _tamper(rnd, rows[2], [1])
    for got in (r.check_batch(F.rows_array(rows)), _device(r, F.rows_array(rows))):
        assert got[0].tolist() == [SAT, SAT, 0] and got[1].tolist() == [0, 0, 1]
    assert F.check(P.constraints[:1], rows[2]) == (0, 1)


def test_zero_constraints_and_zero_batch(pkg):
    import torch
    rnd = random.Random(107)
    r0 = _r1cs(4, [])
    rows = F.rows_array([[1] + [rnd.randrange(R) for _ in range(3)] for _ in range(5)])
    for t in (0, 1, 64):
        r0.set_tile_width(t)
        for got in (r0.check_batch(rows), _device(r0, rows)):
            assert (got[0] == SAT).all() and (got[1] == 0).all()
    assert r0.check_wtns(bytes(PKG.wtns_from_witness([1, 2, 3, 4]))) == (SAT, 0)
    r1 = _r1cs(4, [({1: 1}, {2: 1}, {3: 1})])
    empty = np.zeros((0, 4, 32), dtype=np.uint8)
    first, nfail = r1.check_batch(empty)
    assert first.shape == (0,) and nfail.shape == (0,)
    first, nfail = r1.check_batch_device(torch.zeros((0, 4, 32), dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert tuple(first.shape) == (0,) and tuple(nfail.shape) == (0,)


def test_large_system_strides(pkg):
    """>= 100 000 constraints: every wave strides over its constraint groups several times.  The system is 100 scaled copies
    (k A, B, k C) of a planted base, copy-major, so a base constraint fails in a row exactly when all its copies do."""
    rnd = random.Random(108)
    nb, copies = 1000, 100
    shapes = [dict(a=rnd.randint(1, 6), b=rnd.randint(0, 4), c=rnd.randint(0, 5), dup=rnd.random() < 0.2) for _ in range(nb)]
    P = F.planted_system(rnd, 64, shapes, [1, R - 1, 2, None])
    base = P.constraints
    cons = list(base)
    for _ in range(copies - 1):
        ks = [rnd.randrange(1, R) for _ in range(nb)]
        cons += [([(w, c * k % R) for w, c in a], b, [(w, c * k % R) for w, c in c_]) for (a, b, c_), k in zip(base, ks)]
    r = _r1cs(P.n_wires, cons)
    assert r.info["n_constraints"] == nb * copies
    distinct = [P.complete(rnd) for _ in range(8)]
    rows = [list(distinct[s % 8]) for s in range(1000)]
    tampered = sorted(rnd.sample(range(1000), 7)) + [999]
    for s in tampered:
        _tamper(rnd, rows[s], [rnd.choice(P.free), 1 + rnd.randrange(nb)])
    first, nfail = np.full(1000, SAT, dtype=np.uint32), np.zeros(1000, dtype=np.uint32)
    for s in tampered:
        f, n = F.check(base, rows[s])
        first[s], nfail[s] = f, n * copies
    assert nfail[999] >= copies
    sampled = tampered[0]
    assert F.check(cons, rows[sampled]) == (first[sampled], nfail[sampled])
    assert F.check(cons, rows[1]) == (SAT, 0)
    for batch in (64, 1000):
        arr = F.rows_array(rows[:batch])
        for t in (0, 1, 64) if batch == 1000 else (0, 8):
            r.set_tile_width(t)
            got = _device(r, arr)
            assert np.array_equal(got[0], first[:batch]) and np.array_equal(got[1], nfail[:batch]), (batch, t)
    r.set_tile_width(0)
    got = r.check_batch(F.rows_array(rows[:64]))
    assert np.array_equal(got[0], first[:64]) and np.array_equal(got[1], nfail[:64])


# -- 6. every entry point on the same rows ---------------------------------------------------------------------------------
def test_entry_points_agree(pkg, tmp_path):
    rnd = random.Random(109)
    small = (0, 1, 2, 3, 5, 8)
    shapes = [dict(a=rnd.choice(small), b=rnd.choice(small), c=rnd.choice(small), dup=True, edge=True) for _ in range(150)]
    P = F.planted_system(rnd, 10, shapes, EDGE_POOL)
    cons = P.constraints
    r = _r1cs(P.n_wires, cons)
    (tmp_path / "c.r1cs").write_bytes(F.write_r1cs(P.n_wires, cons))
    rows = [P.complete(rnd) for _ in range(6)]
    tampered = [1, 2, 5]
    for s in tampered:
        _tamper(rnd, rows[s], rnd.sample(range(1, P.n_wires), 1 + s))
    want = _expect(cons, rows, tampered)
    assert all(want[1][s] >= 1 for s in tampered)
    canon = F.rows_array(rows)
    results = {"host": r.check_batch(canon), "device": _device(r, canon),
               "montgomery": _device(r, F.rows_array(_mont_rows(rows)), montgomery=True)}
    for name, got in results.items():
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
    cli = os.path.join(os.path.dirname(PKG.R1CS_LIB_PATH), "check-witness")
    for s, row in enumerate(rows):
        wtns = bytes(PKG.wtns_from_witness(row))
        assert r.check_wtns(wtns) == (want[0][s], want[1][s]), s
        (tmp_path / "w.wtns").write_bytes(wtns)
        p = subprocess.run([cli, str(tmp_path / "c.r1cs"), str(tmp_path / "w.wtns")], capture_output=True, text=True, timeout=120)
        if want[0][s] == SAT:
            assert p.returncode == 0 and "satisfies all constraints" in p.stdout, p.stdout + p.stderr
        else:
            msg = "constraint %d not satisfied (%d constraints fail)" % (want[0][s], want[1][s])
            assert p.returncode == 1 and msg in p.stdout, p.stdout + p.stderr
