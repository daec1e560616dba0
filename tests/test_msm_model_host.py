"""The host model of the prover's MSM bookkeeping (tests/msm_model.py) against plain integers, and the census of the scalar rows
that tests/test_gpu_groth16_msm.py sends to the GPU (tests/msm_fixtures.py): every digit event and every chunk event named below
occurs at every window width c = 7 .. 15 on the wire side and at every domain of the H side, checked here without a GPU.
Run with -s to see the counts."""
import os
import random
import subprocess

import numpy as np
import pytest

from tests import msm_fixtures as MF
from tests import msm_model as M
from tests import qap_reference as QR

R = M.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# n_sc, c, windows, buckets per window, buckets per reduce_kernel lane
SHAPE_TABLE = [(1, 7, 37, 64, 1), (2047, 7, 37, 64, 1), (2048, 8, 32, 128, 2), (4095, 8, 32, 128, 2), (4096, 9, 29, 256, 4), (8192, 10, 26, 512, 8),
               (16384, 11, 24, 1024, 16), (32768, 12, 22, 2048, 32), (65536, 13, 20, 4096, 64), (131072, 14, 19, 8192, 128),
               (262143, 14, 19, 8192, 128), (262144, 15, 17, 16384, 256), (1 << 20, 15, 17, 16384, 256), (1 << 27, 15, 17, 16384, 256)]


def test_shape_table():
    for n_sc, c, n_win, n_b, per in SHAPE_TABLE:
        s = M.msm_shape(n_sc)
        assert (s.c, s.n_win, s.n_b, s.per_lane) == (c, n_win, n_b, per), s
        assert s.n_win * s.c >= 254 > (s.n_win - 1) * s.c  # the last window starts below bit 254
    assert {M.msm_shape(n).c for n in MF.WIRE_SIZES} == set(range(7, 16))
    assert [M.msm_shape(1 << p).c for p in MF.H_POWERS] == list(range(8, 16))
    assert MF.P >= 1024 and all(MF.P % (1 << (c - 1)) for c in range(7, 16))


@pytest.mark.parametrize("c", range(7, 16))
def test_digits_recombine(c):
    """0, 1, r - 1, 2^253, 2^253 - 1, the edge scalars of this c and 3000 random scalars: the digits are in range, recombine to the
    scalar, and the numpy recoding gives the same digits and keys as the integer one"""
    shape = M.shape_of_c(c)
    rnd = random.Random(c)
    edges, _ = MF.edge_scalars(shape)
    ks = [0, 1, R - 1, 1 << 253, (1 << 253) - 1] + edges + [rnd.randrange(R) for _ in range(3000)]
    ks += [rnd.randrange(1 << rnd.randrange(1, 254)) for _ in range(500)]
    raw, cin, dig = M.recode(M.scalars_array(ks), shape)
    for j, k in enumerate(ks):
        d = M.digits(k, c, shape.n_win)
        assert len(d) == shape.n_win and all(-shape.n_b + 1 <= x <= shape.n_b for x in d)
        assert sum(x << (c * w) for w, x in enumerate(d)) == k
        assert d == [int(x) for x in dig[:, j]], hex(k)
        assert M.raw_windows(k, c, shape.n_win) == [int(x) for x in raw[:, j]]
    # keys and their order: two rows of a short list by both routes
    small = M.Shape(len(ks[:200]))
    assert small.c == 7
    rows = [ks[:200], ks[200:400]]
    keys, vals = M.sorted_entries(small, [M.recode(M.scalars_array(r), small)[2] for r in rows])
    want = sorted(M.keys_of(small, rows), key=lambda kv: kv[0])  # (stable)
    assert [(int(a), int(b)) for a, b in zip(keys, vals)] == want
    assert max(k for k, _ in want) < 2 * small.n_win * small.n_b


def test_level_count_ends():
    """run_msm's loop: bounds n, 2 ceil(n / 32), ... fall strictly until one chunk is left; the depth at the sizes used"""
    for n in list(range(1, 5000)) + [(1 << k) + d for k in range(12, 33) for d in (-1, 0, 1)] + [0xffffffff]:
        b = M.level_bounds(n)
        assert b[-1] <= M.K and all(x > y for x, y in zip(b, b[1:])) and len(b) <= 8
    assert len(M.level_bounds(32)) == 1 and len(M.level_bounds(33)) == 2 and len(M.level_bounds(2 * 17 * 262144)) == 6


def test_chunk_census_on_a_hand_made_list():
    """64 + 32 + 1 + 31 + 100 entries: runs and seams counted by hand"""
    keys = np.repeat(np.arange(5, dtype=np.uint32), [64, 32, 1, 31, 100])
    cen = M.chunk_census(keys, keys.size + 40)
    l0 = cen["levels"][0]
    # run 0: chunks 0, 1 whole; run 1: chunk 2 whole; runs 2, 3: chunk 3; run 4: chunks 4 .. 6 and 4 entries of chunk 7
    assert (l0["run_ends_on_seam"], l0["run_starts_on_seam"], l0["run_over_3_chunks"]) == (3, 3, 1)
    assert l0["chunks"] == 8 and l0["partials"] == 2 + 4 and l0["head_and_tail_partial"] == 0 and l0["head_then_complete"] == 0
    assert [lv["entries"] for lv in cen["levels"]] == [228, 6] and cen["launches"] == 2
    keys = np.repeat(np.arange(4, dtype=np.uint32), [40, 10, 30, 40])
    l0 = M.chunk_census(keys, keys.size)["levels"][0]
    # chunk 1: the tail of run 0 (8), run 1 whole, the head of run 2 (14): head and tail partial, and a complete run between;
    # chunk 2: the tail of run 2 (16) and the head of run 3 (16): head and tail partial with nothing between
    assert l0["head_and_tail_partial"] == 2 and l0["head_then_complete"] == 1 and l0["partials"] == 1 + 2 + 2 + 1


def _show(title, cen, extra=""):
    lv = cen["chunks"]["levels"]
    print("%s: entries %s, partials %s, launches %d; level 0: %s%s" % (
        title, [x["entries"] for x in lv], [x["partials"] for x in lv], cen["chunks"]["launches"],
        ", ".join("%s %d" % (e, lv[0][e]) for e in M.CHUNK_EVENTS), extra))


def _check_chunks(cen, min_levels, events=M.CHUNK_EVENTS):
    l0 = cen["chunks"]["levels"][0]
    for e in events:
        assert l0[e] >= 1, e
    assert len(cen["chunks"]["levels"]) >= min_levels


@pytest.mark.parametrize("n_sc", MF.WIRE_SIZES)
def test_census_of_the_wire_rows(n_sc):
    shape, n_vars, inf, rows, rs = MF.wire_case(n_sc)
    names = [name for name, _ in rows]
    lists = MF.scalar_lists(rows, rs)
    cen = M.call_census(shape, lists, MF.N_PUB + 1, n_vars)
    c, n_b, n_win, mid = shape.c, shape.n_b, shape.n_win, shape.n_win // 2
    # digit events of the edge row: in window 0, a middle window, the one before the top, and the top one where the scalar is below r
    edges, expected = MF.edge_scalars(shape)
    got = cen["digits"][names.index("digit edges")]
    for e in ("top_bucket", "most_negative"):
        assert {0, mid, n_win - 2} <= expected[e] <= set(got[e]), e
    for e in ("top_bucket_by_carry", "zero_with_carry"):
        assert {mid, n_win - 2} <= expected[e] <= set(got[e]), e
    wide = {w for w in range(n_win - 1) if M.straddles(c, w)}   # (the top window's n_b + 1 need not be below r)
    assert (wide or c == 8) and wide <= expected["straddle"] <= set(got["straddle"])  # (windows of 8 bits never straddle)
    for e in ("carry_chain", "top_max", "top_max_carry", "zero_scalar"):
        assert expected[e] >= 1 and got[e] >= expected[e], e
    assert got["negative"] > 0 and all(x in edges for x in (0, 1, R - 1, 1 << 253, (1 << 253) - 1))
    # the sweeps fill every bucket of their window, the first and the last of every reduce_kernel lane among them
    keys = cen["keys"]
    for w in (0, mid):
        for tag in ("", ", negated"):
            row = names.index("bucket sweep, window %d%s" % (w, tag))
            first = (row * n_win + w) * n_b
            present = np.unique(keys[(keys >= first) & (keys < first + n_b)]) - first
            if not tag:
                assert present.size == n_b
            else:
                assert cen["digits"][row]["negative"] >= n_vars // 2
    for tag in ("single bucket n_b", "single bucket n_b 2^c + 1"):
        d = cen["digits"][names.index(tag)]
        assert d["top_bucket"] == ([0] if tag.endswith("n_b") else [1]) and d["entries"] >= n_vars
    # equal bases: buckets of exactly +i, -(i + P) and of +i, +(i + P)
    cancel, double = M.pair_runs(keys, cen["vals"], MF.P)
    assert cancel >= MF.CANCEL_WIRES and double >= MF.CANCEL_WIRES
    assert cen["digits"][names.index("cancellation and doubling")]["zero_scalar"] > n_vars // 2
    # buckets that hold only scalars outside the C MSM's range stay at infinity there
    assert cen["outside"] >= 1
    if inf:
        idx, sign = cen["vals"] & np.uint32(M.SIGN - 1), cen["vals"] >> np.uint32(31)
        under = np.isin(idx, np.array(inf, dtype=np.uint32))
        assert (under & (sign == 1)).any() and (under & (sign == 0)).any()
    assert ("infinity bases" in names) == (c in (9, 15) and n_sc in (4096, 262144))
    assert ("all ones" in names) == (n_sc in (2048, 262144))
    _check_chunks(cen, 4 if n_sc == 262144 else 3)
    _show("wire side n_sc %d c %d, rows: %s" % (n_sc, c, "; ".join(names)), cen,
          "; cancelling buckets %d, doubling %d, buckets outside C's range %d" % (cancel, double, cen["outside"]))
    print("    digit edges: " + ", ".join("%s %s" % (e, got[e]) for e in list(M.DIGIT_EVENTS) + ["carry_chain", "top_max", "top_max_carry", "zero_scalar"]))


@pytest.mark.parametrize("n_sc", (2048, 16384))
def test_census_of_the_batches_of_five(n_sc):
    shape = M.msm_shape(n_sc)
    rows = MF.batch5_rows(shape, n_sc - 2, 7000 + n_sc)
    cen = M.call_census(shape, MF.scalar_lists(rows, MF.rs_pairs(5, 7 + n_sc)), MF.N_PUB + 1, n_sc - 2)
    assert int(cen["keys"].max()) >= 4 * shape.n_win * shape.n_b  # the key carries the row
    _check_chunks(cen, 3)
    _show("batch of five n_sc %d c %d" % (n_sc, shape.c), cen)


@pytest.mark.parametrize("p", MF.H_POWERS)
def test_census_of_the_constant_quotient(p):
    """two rows of n scalars r - 2: per window one bucket with all n entries, so every run starts and ends on a seam and is
    summed over n / 32 chunks and at least three levels (four at 2^18); the seams inside runs of other lengths are the planted
    rows' (below) and the wire side's"""
    n = 1 << p
    shape = M.msm_shape(n)
    assert shape.c == p - 3
    cen = M.call_census(shape, [[R - 2] * n] * 2)
    l0 = cen["chunks"]["levels"][0]
    live = sum(1 for d in M.digits(R - 2, shape.c, shape.n_win) if d)
    assert l0["run_ends_on_seam"] == l0["run_starts_on_seam"] == l0["run_over_3_chunks"] == 2 * live
    assert l0["partials"] == l0["chunks"] == 2 * live * n // M.K
    assert len(cen["chunks"]["levels"]) >= (4 if p == 18 else 3)
    _show("H side constant quotient n 2^%d c %d" % (p, shape.c), cen)


@pytest.mark.parametrize("p", MF.PLANTED_POWERS)
def test_census_of_the_planted_quotients(p):
    """h of the planted systems (three rows, c = 8 and 9) is uniform below r: runs of about 16 entries at every offset to the
    seams, so every chunk event but the run over three whole chunks, which the constant quotient of the same domain (above) has
    in every window"""
    n = 1 << p
    shape = M.msm_shape(n)
    pl, _, rows, hs = MF.planted_case(p)
    assert all(len(h) == n for h in hs) and M.msm_shape(pl.n_wires + 2).c == shape.c  # (here both MSM shapes have one width)
    cen = M.call_census(shape, hs)
    _check_chunks(cen, 2, [e for e in M.CHUNK_EVENTS if e != "run_over_3_chunks"])
    assert cen["chunks"]["launches"] >= 3 and sum(d["negative"] for d in cen["digits"]) > n
    _show("H side planted quotient n 2^%d c %d" % (p, shape.c), cen)


def test_constant_quotient_closed_form():
    """section 4 of the constant-quotient keys against the witness map's reference at n = 2, 4, 32: h_j = -2 w_0^2"""
    rnd = random.Random(5)
    for p in (1, 2, 5):
        n = 1 << p
        ent = MF.constant_quotient(p)
        for w0 in (1, rnd.randrange(R)):
            w = [w0] + [rnd.randrange(R) for _ in range(5)]
            a, b = [0] * n, [0] * n
            for m, k, s, v in ent:
                (b if m else a)[k] = ((b if m else a)[k] + v * w[s]) % R
            c = [x * y % R for x, y in zip(a, b)]
            want = [-2 * w0 * w0 % R] * n
            assert QR.h_ntt(a, b, c) == want and (p > 2 or QR.h_direct(a, b, c) == want)


def test_group_law_harness_compiles_for_gfx950(tmp_path):
    """compile only (no GPU here): the harness of tests/test_gpu_bn254_group.py must not arrive uncompilable"""
    src = os.path.join(ROOT, "tests", "native", "bn254_group.hip")
    p = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "-I" + os.path.join(ROOT, "circom-witnesscalc_amd", "r1cs"), src, "-o", str(tmp_path / "bn254_group")],
                       capture_output=True, text=True, timeout=1800)
    assert p.returncode == 0, p.stderr[-4000:]
