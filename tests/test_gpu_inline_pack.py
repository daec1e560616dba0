"""The divider wave packs witness rows between its requests (kernels.hip, pack_schedule.cc): the rows are the bytes of the C
oracle and of the same call with CWC_INLINE_PACK=0 (every row left to the pack kernel).  The output buffer is filled with
0xA5 before every call.  CWC_INLINE_PACK=2 gives the divider waves everything that is ready in front of the last request
(small graphs: the schedule's own prefix would leave them little), 1 the prefix of the schedule."""
import random

import numpy as np
import pytest

from oracle import cbind, model
import cwc_import
C = cwc_import.load().graphgen.circuits
Builder = cwc_import.load().graphgen.builder.Builder

pytestmark = pytest.mark.gpu
M = model.M
DIVIDER = 0x100
EDGE = [0, 1, 2, 3, 255, 256, M - 1, M - 2, M // 2, M // 2 + 1, 1 << 253, (1 << 64) - 1, 1 << 64, (1 << 128) - 1, 1 << 200]


def _rand_row(rnd, n, small=0.3):
    return [1] + [rnd.randrange(M) if rnd.random() > small else rnd.choice([rnd.randrange(1 << 16), rnd.choice(EDGE)]) for _ in range(n - 1)]


def _device_call(g, inp, monkeypatch, mode, montgomery=False):
    import torch
    monkeypatch.setenv("CWC_INLINE_PACK", mode)
    n = inp.shape[0]
    d_in = torch.from_numpy(inp).cuda()
    d_out = torch.full((n, g.n_witness, 32), 0xA5, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g.calc_witness_batch_device(d_in, d_out, d_st, montgomery=montgomery)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_st.cpu().numpy()


def _check(pkg, data, rows, keys, monkeypatch, modes=("2", "1"), oracle_rows=None):
    g = pkg.Graph(data)
    inp = cbind.ints_to_array(rows) if not isinstance(rows, np.ndarray) else rows
    sel = np.arange(inp.shape[0]) if oracle_rows is None else np.asarray(oracle_rows)
    want, wst = cbind.Graph(data).evaluate_batch(inp[sel])
    for key in keys:
        g.set_tile_width(key)
        base, bst = _device_call(g, inp, monkeypatch, "0")
        assert np.array_equal(bst[sel] != 0, wst != 0), hex(key)
        ok = wst == 0
        assert np.array_equal(base[sel][ok], want[ok]), hex(key)
        for mode in modes:
            got, st = _device_call(g, inp, monkeypatch, mode)
            assert np.array_equal(st, bst), (hex(key), mode)
            assert np.array_equal(got, base), (hex(key), mode)
    return g


@pytest.mark.parametrize("waves", ["1", "4"])
@pytest.mark.parametrize("key", [1 | DIVIDER, 2 | DIVIDER, 4 | DIVIDER])
def test_gadget_graph_batches_and_workgroup_shapes(pkg, monkeypatch, key, waves):
    monkeypatch.setenv("CWC_WAVES_PER_WORKGROUP", waves)
    rnd = random.Random(31 + key)
    data = C.build_gadgets().to_bin()
    assert pkg.Graph(data).pack_schedule(key)[1][-1] > 0  # (the program has rows for the divider waves)
    for n in (1, 2, 3, 5, 37, 96):
        _check(pkg, data, [_rand_row(rnd, 7) for _ in range(n)], (key,), monkeypatch)


def test_sets_that_end_with_an_error_status(pkg, monkeypatch):
    """A division chain beside a shift that overflows for some sets (status bit 0): those sets' statuses and the rows of
    the others are what the pack kernel alone gives."""
    rnd = random.Random(77)
    b = Builder()
    x, y = b.input("x", 2)
    one = b.const(1)
    b.signal(b.op("Shl", x, one))
    v = x
    for step in range(12):
        v = b.signal(b.div(b.add(b.mul(v, v), one), b.add(v, y)))
        b.signal(b.add(v, x))
    data = b.to_bin()
    rows = [[1, rnd.choice([M // 2 + 5, rnd.randrange(1 << 200), 3]), rnd.randrange(M)] for _ in range(100)]
    _, wst = cbind.Graph(data).evaluate_batch(cbind.ints_to_array(rows))
    assert (wst != 0).any() and (wst == 0).any(), "the batch must hold sets of both kinds"
    _check(pkg, data, rows, (1 | DIVIDER, 2 | DIVIDER, 4 | DIVIDER), monkeypatch)


@pytest.mark.parametrize("batch", [1024, 1023])
def test_authv2_class_graph(pkg, monkeypatch, batch):
    data = C.build_authv2_class().to_bin()
    g0 = pkg.Graph(data)
    rng = np.random.default_rng(batch)
    inp = np.frombuffer(rng.bytes(batch * g0.n_inputs * 32), dtype=np.uint8).reshape(batch, g0.n_inputs, 32).copy()
    inp[:, :, 31] &= 0x1F
    inp[:, 0, :] = 0
    inp[:, 0, 0] = 1
    g = _check(pkg, data, inp, (0,), monkeypatch, modes=("1", "2"), oracle_rows=[0, 1, 2, 3, 511, batch - 2, batch - 1])
    assert g.last_timing()["divider"] == 1 and g.last_timing()["streams"] == 1  # (the cost model's choice is in scope)


def test_montgomery_rows_of_the_prover_handoff(pkg, monkeypatch):
    rnd = random.Random(41)
    data = C.build_gadgets().to_bin()
    rows = [_rand_row(rnd, 7) for _ in range(70)]
    inp = cbind.ints_to_array(rows)
    want, wst = cbind.Graph(data).evaluate_batch(inp)
    g = pkg.Graph(data)
    rinv = pow(1 << 256, -1, M)
    for key in (1 | DIVIDER, 2 | DIVIDER, 4 | DIVIDER):
        g.set_tile_width(key)
        base, bst = _device_call(g, inp, monkeypatch, "0", montgomery=True)
        for s in np.nonzero(wst == 0)[0][:5]:
            assert [v * rinv % M for v in cbind.array_to_ints(base[s])] == cbind.array_to_ints(want[s])
        for mode in ("2", "1"):
            got, st = _device_call(g, inp, monkeypatch, mode, montgomery=True)
            assert np.array_equal(got, base) and np.array_equal(st, bst), (hex(key), mode)


def test_chunked_workspaces_and_several_launches(pkg, monkeypatch):
    rnd = random.Random(12)
    data = C.build_gadgets().to_bin()
    rows = [_rand_row(rnd, 7) for _ in range(301)]
    monkeypatch.setenv("CWC_WORKSPACE_GB", "0.0002")
    for streams in (None, "1", "3"):
        if streams is None:
            monkeypatch.delenv("CWC_STREAMS", raising=False)
        else:
            monkeypatch.setenv("CWC_STREAMS", streams)
        g = _check(pkg, data, rows, (2 | DIVIDER, 4 | DIVIDER), monkeypatch)
        if streams == "1":
            assert g.last_timing()["n_launches"] >= 4


def test_five_calls_without_synchronisation(pkg, monkeypatch):
    """One handle, one stream, one output buffer per call: call i + 1's divider waves touch their own rows only."""
    import torch
    monkeypatch.setenv("CWC_INLINE_PACK", "2")
    rnd = random.Random(5)
    data = C.build_gadgets().to_bin()
    g = pkg.Graph(data)
    og = cbind.Graph(data)
    g.set_tile_width(2 | DIVIDER)
    jobs = []
    for i in range(5):
        rows = cbind.ints_to_array([_rand_row(rnd, 7) for _ in range(96)])
        jobs.append((rows, torch.from_numpy(rows).cuda(), torch.full((96, g.n_witness, 32), 0xA5, dtype=torch.uint8, device="cuda"), torch.zeros(96, dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    for rows, d_in, d_out, d_st in jobs:
        g.calc_witness_batch_device(d_in, d_out, d_st)
    torch.cuda.synchronize()
    for rows, d_in, d_out, d_st in jobs:
        want, wst = og.evaluate_batch(rows)
        ok = wst == 0
        assert np.array_equal(d_st.cpu().numpy() != 0, wst != 0) and np.array_equal(d_out.cpu().numpy()[ok], want[ok])


def test_rows_produced_right_in_front_of_a_request_are_fresh(pkg, monkeypatch):
    """A chain in which the operands of every division, and a witness signal beside them, are produced one to three
    operations in front of the division: a row counted ready one request too early is read before its store has completed
    and shows as a wrong row.  Two different batches through one handle, so that a stale read finds the other batch's value."""
    rnd = random.Random(91)
    b = Builder()
    xs = b.input("x", 4)
    one = b.const(1)
    for lag in (1, 2, 3):
        for x in xs:
            v = x
            for step in range(24):
                fresh = [b.add(b.mul(v, v), one)]
                for _ in range(lag - 1):
                    fresh.append(b.add(fresh[-1], x))
                b.signal(fresh[0])                      # a witness row produced `lag` operations in front of the request
                den = b.signal(fresh[-1])
                v = b.signal(b.div(b.add(fresh[0], one), den))
    data = b.to_bin()
    g = pkg.Graph(data)
    og = cbind.Graph(data)
    for key in (1 | DIVIDER, 2 | DIVIDER, 4 | DIVIDER):
        g.set_tile_width(key)
        assert g.pack_schedule(key)[1][-1] > 0
        for rep in range(3):
            inp = cbind.ints_to_array([[1] + [rnd.randrange(M) for _ in range(4)] for _ in range(70)])
            want, wst = og.evaluate_batch(inp)
            assert not wst.any()
            for mode in ("2", "1"):
                got, st = _device_call(g, inp, monkeypatch, mode)
                assert not st.any() and np.array_equal(got, want), (hex(key), rep, mode)
