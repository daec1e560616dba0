"""The R1CS check on an MI355X (include/graph_witness_r1cs.h): witness batches of the product checked against R1CS derived from the
generator's circuits (tests/r1cs_fixtures.py), compared with the big-integer checker."""
import os
import random
import subprocess

import numpy as np
import pytest

import cwc_import
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
C = PKG.graphgen.circuits
SAT = 0xFFFFFFFF

pytestmark = pytest.mark.gpu


def _poseidon_builder(n=2):
    """circomlib Poseidon(n) with its intermediate signals as wires (what circom keeps of x^5 rounds and mixes)"""
    b = PKG.graphgen.builder.Builder()
    ins = b.input("inputs", n)
    for h in ins:
        b.signal(h)
    b.signal(C.poseidon(b, ins, signals=True, circomlib=True))
    return b


def _field_rows(n_inputs, batch, seed):
    from tools.synth import synth_inputs
    return synth_inputs("field", n_inputs, batch, seed)


def _circuit(b):
    cons = F.derive_r1cs(b)
    return PKG.Graph(b.to_bin()), cons, PKG.R1cs(F.write_r1cs(len(b._witness), cons))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _tamper(rows, s, wire, rnd):
    v = rnd.randrange(1, F.R)
    old = int.from_bytes(bytes(rows[s, wire]), "little")
    rows[s, wire] = np.frombuffer(((old + v) % F.R).to_bytes(32, "little"), dtype=np.uint8)


def test_poseidon_batch_satisfied_at_tile_widths(pkg):
    g, cons, r = _circuit(_poseidon_builder())
    wit, st = g.calc_witness_batch(_field_rows(g.n_inputs, 256, 21))
    assert not st.any()
    assert F.check(cons, F.row_ints(wit[0])) == (SAT, 0)
    for t in (1, 8, 64):
        r.set_tile_width(t)
        first, nfail = r.check_batch((wit, st))
        assert (first == SAT).all() and (nfail == 0).all(), t


def test_tampered_set_is_found_exactly(pkg):
    b = _poseidon_builder()
    g, cons, r = _circuit(b)
    wit, st = g.calc_witness_batch(_field_rows(g.n_inputs, 200, 22))
    in_ab = {w for a, bb, _ in cons for w in list(a) + list(bb)}
    c_only = [w for w in range(1, g.n_witness) if w not in in_ab and any(w in c for _, _, c in cons)]
    assert c_only
    rnd = random.Random(3)
    for wire, s in ((0, 17), (1, 199), (g.n_witness - 1, 0), (c_only[0], 123), (c_only[-1], 64)):
        rows = wit.copy()
        _tamper(rows, s, wire, rnd)
        want = F.check(cons, F.row_ints(rows[s]))
        assert want[1] >= 1
        for t in (0, 8, 64):
            r.set_tile_width(t)
            first, nfail = r.check_batch(rows)
            bad = np.flatnonzero(nfail)
            assert list(bad) == [s], (wire, t, bad)
            assert (int(first[s]), int(nfail[s])) == want, (wire, t)
            assert (first[np.arange(200) != s] == SAT).all()


def test_zero_divisor_makes_the_proof_invalid(pkg):
    """The reference's graph.rs division comment: `inv <-- 1/x` gives 0 for x = 0, and `x * inv === 1` fails in those sets only,
    while the witness calculator's status words stay 0."""
    b = PKG.graphgen.builder.Builder()
    x, y = b.input("x", 1)[0], b.input("y", 1)[0]
    b.signal(x)
    b.signal(y)
    b.signal(b.mul(x, y))                                  # constraint 0: x * y = xy
    inv = b.signal(b.div(b.const(1), x))                    # a hint: no constraint
    b.signal(b.add(b.mul(y, y), x))                         # constraint 1
    cons = F.derive_r1cs(b, extra=[({x: 1}, {inv: 1}, {-1: 1})])  # constraint 2: x * inv === 1
    assert len(cons) == 3
    g, r = PKG.Graph(b.to_bin()), PKG.R1cs(F.write_r1cs(len(b._witness), cons))
    rows = _field_rows(g.n_inputs, 300, 23)
    zero_sets = [0, 5, 63, 64, 200, 299]
    rows[zero_sets, 1] = 0
    wit, st = g.calc_witness_batch(rows)
    assert not st.any()
    for t in (0, 1, 64):
        r.set_tile_width(t)
        first, nfail = r.check_batch(wit)
        assert list(np.flatnonzero(nfail)) == zero_sets
        assert (first[zero_sets] == 2).all() and (nfail[zero_sets] == 1).all()
        for s in zero_sets[:2]:
            assert F.check(cons, F.row_ints(wit[s])) == (2, 1)


def test_montgomery_rows_chained_on_the_hand_off_event(pkg):
    import torch
    for builder, zero_sets in ((_poseidon_builder(), []), (None, [3, 90])):
        if builder is None:  # the zero-divisor circuit: answers that are not all "satisfied"
            builder = PKG.graphgen.builder.Builder()
            x = builder.input("x", 1)[0]
            builder.signal(x)
            inv = builder.signal(builder.div(builder.const(1), x))
            cons = F.derive_r1cs(builder, extra=[({x: 1}, {inv: 1}, {-1: 1})])
        else:
            cons = F.derive_r1cs(builder)
        g, r = PKG.Graph(builder.to_bin()), PKG.R1cs(F.write_r1cs(len(builder._witness), cons))
        rows = _field_rows(g.n_inputs, 130, 24)
        rows[zero_sets, 1] = 0
        d_in = torch.from_numpy(rows).cuda()
        d_w = torch.empty((130, g.n_witness, 32), dtype=torch.uint8, device="cuda")
        d_m = torch.empty_like(d_w)
        d_st = torch.zeros(130, dtype=torch.int32, device="cuda")
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        g.calc_witness_batch_device(d_in, d_w, d_st, stream=s1)
        f_can, n_can = r.check_batch_device(d_w, stream=s1)
        ev = torch.cuda.Event()
        g.calc_witness_batch_device(d_in, d_m, d_st, stream=s1, montgomery=True, done_event=ev)
        s2.wait_event(ev)
        f_mont, n_mont = r.check_batch_device(d_m, stream=s2, montgomery=True)
        torch.cuda.synchronize()
        assert not d_st.any()
        assert not torch.equal(d_w, d_m)
        assert np.array_equal(_u32(f_can), _u32(f_mont)) and np.array_equal(_u32(n_can), _u32(n_mont))
        assert list(np.flatnonzero(_u32(n_can))) == zero_sets
        # Montgomery rows read as canonical ones are (almost surely) not a witness
        f_wrong, _ = r.check_batch_device(d_m)
        torch.cuda.synchronize()
        assert (_u32(f_wrong) != SAT).all()


def test_authv2_class_batch_at_scale(pkg):
    import torch
    with F.gadget_constraints():
        b = C.build_authv2_class()
    g, cons, r = _circuit(b)
    batch = 1024
    d_in = torch.from_numpy(_field_rows(g.n_inputs, batch, 25)).cuda()
    d_w = torch.empty((batch, g.n_witness, 32), dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(batch, dtype=torch.int32, device="cuda")
    g.calc_witness_batch_device(d_in, d_w, d_st)
    first, nfail = r.check_batch_device(d_w)
    torch.cuda.synchronize()
    assert not d_st.any()
    assert (_u32(first) == SAT).all() and (_u32(nfail) == 0).all()
    # a few hundred random constraints of every set, in the big-integer checker, on the wires they read
    rnd = random.Random(8)
    sample = rnd.sample(range(len(cons)), 300)
    wires = sorted({w for j in sample for lc in cons[j] for w in lc})
    cols = d_w[:, torch.tensor(wires, device="cuda")].cpu().numpy()
    for s in range(0, batch, 7):
        w = dict(zip(wires, F.row_ints(cols[s])))
        assert F.check(cons, w, sample) == (SAT, 0), s
    # 16 tampered sets, each at a wire some constraint reads
    used = sorted({w for con in cons for lc in con for w in lc if w})
    sets = sorted(rnd.sample(range(batch), 16))
    for s in sets:
        wire = rnd.choice(used)
        v = (int.from_bytes(bytes(d_w[s, wire].cpu().numpy()), "little") + rnd.randrange(1, F.R)) % F.R
        d_w[s, wire] = torch.from_numpy(np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8).copy()).cuda()
    first, nfail = r.check_batch_device(d_w)
    torch.cuda.synchronize()
    first, nfail = _u32(first), _u32(nfail)
    assert list(np.flatnonzero(nfail)) == sets
    for s in sets:
        assert (int(first[s]), int(nfail[s])) == F.check(cons, F.row_ints(d_w[s].cpu().numpy())), s


def test_wtns_files(pkg, tmp_path):
    g, cons, r = _circuit(_poseidon_builder())
    wit, st = g.calc_witness_batch(_field_rows(g.n_inputs, 2, 26))
    _tamper(wit, 1, 7, random.Random(4))
    PKG.wtns_save_batch(wit, str(tmp_path / "w_%lu.wtns"))
    want = F.check(cons, F.row_ints(wit[1]))
    assert want[1] >= 1
    (tmp_path / "c.r1cs").write_bytes(F.write_r1cs(g.n_witness, cons))
    good, bad = (tmp_path / "w_0.wtns").read_bytes(), (tmp_path / "w_1.wtns").read_bytes()
    assert r.check_wtns(good) == (SAT, 0)
    assert r.check_wtns(bad) == want
    cli = os.path.join(os.path.dirname(PKG.R1CS_LIB_PATH), "check-witness")
    p = subprocess.run([cli, str(tmp_path / "c.r1cs"), str(tmp_path / "w_0.wtns")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([cli, str(tmp_path / "c.r1cs"), str(tmp_path / "w_1.wtns")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and ("constraint %d not satisfied" % want[0]) in p.stdout, p.stdout + p.stderr
