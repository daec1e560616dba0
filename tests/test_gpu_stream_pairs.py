"""Two-stream divider programs as eight-wave workgroups of two tiles (pipeline.cc waves_per_workgroup: [A.s0, A.s1, B.s0, B.s1, their
four divider waves]; the shape of more than 256 tiles, CWC_STREAM_TILES_PER_WORKGROUP=2 forces it for any batch): the witnesses are
the bytes of the C oracle, odd tile counts (a workgroup whose second tile is absent) included."""
import random

import numpy as np
import pytest

from oracle import cbind, model
import cwc_import
C = cwc_import.load().graphgen.circuits

pytestmark = pytest.mark.gpu
M = model.M
DIVIDER, STREAMS2 = 0x100, 0x800
EDGE = [0, 1, 2, 3, 255, 256, M - 1, M - 2, M // 2, M // 2 + 1, 1 << 253, (1 << 64) - 1, 1 << 64, (1 << 128) - 1, 1 << 200]


def _rand_row(rnd, n, small=0.3):
    return [1] + [rnd.randrange(M) if rnd.random() > small else rnd.choice([rnd.randrange(1 << 16), rnd.choice(EDGE)]) for _ in range(n - 1)]


@pytest.mark.parametrize("batch", [1, 2, 3, 1023, 1024, 1025])
def test_authv2_class_graph_at_odd_and_even_tile_counts(pkg, monkeypatch, batch):
    """Key 2 | divider | two streams forced: the oracle's rows for a sample of sets (first, middle, the last tiles), and every row
    equal to the one-stream divider program's (which tests/test_gpu_parity.py and test_gpu_inline_pack.py hold to the oracle)."""
    monkeypatch.setenv("CWC_STREAM_TILES_PER_WORKGROUP", "2")
    data = C.build_authv2_class().to_bin()
    g = pkg.Graph(data)
    rng = np.random.default_rng(batch)
    inp = np.frombuffer(rng.bytes(batch * g.n_inputs * 32), dtype=np.uint8).reshape(batch, g.n_inputs, 32).copy()
    inp[:, :, 31] &= 0x1F
    inp[:, 0, :] = 0
    inp[:, 0, 0] = 1
    sel = sorted({0, batch // 2, max(batch - 4, 0), max(batch - 3, 0), max(batch - 2, 0), batch - 1})
    want, wst = cbind.Graph(data).evaluate_batch(inp[sel])
    assert not wst.any()
    g.set_tile_width(2 | DIVIDER | STREAMS2)
    got, st = g.calc_witness_batch(inp)
    tm = g.last_timing()
    assert tm["streams"] == 2 and tm["divider"] == 1 and tm["tile_width"] == 2
    assert not st.any() and np.array_equal(got[sel], want)
    g.set_tile_width(2 | DIVIDER)
    one, st1 = g.calc_witness_batch(inp)
    assert not st1.any() and np.array_equal(got, one)


def test_default_shape_beyond_256_tiles_is_the_same_program(pkg, monkeypatch):
    """Without the override: 1024 sets run as two-tile workgroups, 400 as one tile per workgroup; same rows either way."""
    monkeypatch.delenv("CWC_STREAM_TILES_PER_WORKGROUP", raising=False)
    data = C.build_authv2_class(scale=0.15).to_bin()
    g = pkg.Graph(data)
    og = cbind.Graph(data)
    rnd = random.Random(3)
    rows = cbind.ints_to_array([_rand_row(rnd, g.n_inputs, small=0.0) for _ in range(515)])
    want, wst = og.evaluate_batch(rows)
    g.set_tile_width(1 | DIVIDER | STREAMS2)  # 515 tiles: two rounds of 256 workgroups, the last one half empty
    got, st = g.calc_witness_batch(rows)
    assert np.array_equal(st != 0, wst != 0) and np.array_equal(got[wst == 0], want[wst == 0])
    g.set_tile_width(2 | DIVIDER | STREAMS2)  # 258 tiles
    got, st = g.calc_witness_batch(rows)
    assert np.array_equal(st != 0, wst != 0) and np.array_equal(got[wst == 0], want[wst == 0])


@pytest.mark.parametrize("key", [1 | DIVIDER | STREAMS2, 2 | DIVIDER | STREAMS2, 4 | DIVIDER | STREAMS2])
def test_gadget_graph_every_op_class(pkg, monkeypatch, key):
    """(the gadget graph has no panicking inputs: the status bits of both panic edges are the forest test's, below)"""
    monkeypatch.setenv("CWC_STREAM_TILES_PER_WORKGROUP", "2")
    rnd = random.Random(17 + key)
    data = C.build_gadgets().to_bin()
    g = pkg.Graph(data)
    og = cbind.Graph(data)
    g.set_tile_width(key)
    for n in (1, 2, 3, 5, 37, 70, 96):
        inp = cbind.ints_to_array([_rand_row(rnd, g.n_inputs) for _ in range(n)])
        want, wst = og.evaluate_batch(inp)
        got, st = g.calc_witness_batch(inp)
        assert np.array_equal(st != 0, wst != 0), (hex(key), n)
        ok = wst == 0
        assert np.array_equal(got[ok], want[ok]), (hex(key), n)


def test_forest_graphs_with_panicking_sets_and_chunked_launches(pkg, monkeypatch):
    monkeypatch.setenv("CWC_STREAM_TILES_PER_WORKGROUP", "2")
    monkeypatch.setenv("CWC_WORKSPACE_GB", "0.0002")
    rnd = random.Random(9)
    seen_bad = seen_ok = 0
    for seed in range(4):
        data = C.build_random_dag(900 + seed, n_ops=200, panic_free=False, parts=2 + seed).to_bin()
        g = pkg.Graph(data)
        og = cbind.Graph(data)
        inp = cbind.ints_to_array([_rand_row(rnd, 7) for _ in range(203)])
        want, wst = og.evaluate_batch(inp)
        for key in (1 | DIVIDER | STREAMS2, 2 | DIVIDER | STREAMS2):
            g.set_tile_width(key)
            got, st = g.calc_witness_batch(inp)
            ok = wst == 0
            assert np.array_equal(st != 0, wst != 0) and np.array_equal(got[ok], want[ok]), (seed, hex(key))
        seen_bad += int((wst != 0).sum())
        seen_ok += int(ok.sum())
    assert seen_bad and seen_ok, "the batches must hold panicking sets and clean ones"
