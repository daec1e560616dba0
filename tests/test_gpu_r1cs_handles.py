"""Who owns what on the device, seen from the handles (R1cs, Groth16, Groth16VerifyingKey over r1cs/device_owners.hpp) on an
MI355X: one handle reused across growing and shrinking batches (and under a small workspace cap) gives, byte for byte, what a
fresh handle gives for that batch alone; the phase timers turn on, report, turn off and go away with their handle; a refused
call leaves the handle as it was; handles are created, used and closed in any order, twice, and unused; and the synchronous
host entry points agree with their device twins at batch 0, 1 and 3.  Ownership bugs show at the first reuse of a handle, not
at size: the circuit has 5 constraints and 2 public signals (domain 2^3), the batches at most 8 rows."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import cwc_import
from tests import groth16_fixtures as GF
from tests import r1cs_fixtures as F
from tests import zkey_coefs_fixtures as ZF

PKG = cwc_import.load()
R = F.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PUB = 2
BATCHES = ((0, 1), (1, 6), (6, 8))  # rows [lo, hi): 1, then 5, then 2
QAP_PHASES = {"evaluation", "inverse_outer", "fused_inner", "forward_outer"}

pytestmark = pytest.mark.gpu


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(*tensors):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


class System:
    """The circuit, its trapdoor key, 8 witness rows with their r, s, and the handles' inputs as files or bytes"""

    def __init__(self):
        rnd = random.Random(2024)
        shapes = [{"a": rnd.randrange(1, 3), "b": rnd.randrange(1, 3), "c": rnd.randrange(0, 2)} for _ in range(5)]
        self.pl = F.planted_system(rnd, 3, shapes, [1, R - 1, 2, None])
        self.r1cs = F.write_r1cs(self.pl.n_wires, self.pl.constraints, n_pub_out=1, n_pub_in=1)
        self.T = GF.Trapdoor(self.pl.constraints, self.pl.n_wires, N_PUB, seed=2024)
        self.zkey = ZF.zkey_of(self.T, ZF.entries_of(self.pl.constraints, N_PUB))  # with the circuit's section 4
        rows = [self.pl.complete(rnd) for _ in range(8)]
        rows[4][self.pl.free[0]] = (rows[4][self.pl.free[0]] + 1) % R  # one row that fails the check
        self.rows = F.rows_array(rows)
        self.rs = np.frombuffer(b"".join(rnd.randrange(R).to_bytes(32, "little") for _ in range(16)), dtype=np.uint8).reshape(8, 2, 32).copy()

    def handles(self):
        """fresh R1cs, Groth16 (from the zkey alone) and Groth16VerifyingKey"""
        return PKG.R1cs(self.r1cs), PKG.Groth16(self.zkey), PKG.Groth16VerifyingKey.from_zkey(self.zkey)

    def publics(self, lo, hi):
        return self.rows[lo:hi, 1:1 + N_PUB]


def run_device(S, handles, lo, hi):
    """rows [lo, hi) through every *_batch_device method -> first_failed, n_failed, h (.r1cs), h (.zkey), proofs, statuses"""
    r, g, vk = handles
    d = _cuda(S.rows[lo:hi])
    first, nfail = r.check_batch_device(d)
    h_r, h_z = r.qap_batch_device(d), g.qap_batch_device(d)
    proofs = g.prove_batch_device(d, rs=S.rs[lo:hi])
    status = vk.verify_batch_device(proofs, _cuda(S.publics(lo, hi)))
    return _host(first, nfail, h_r, h_z, proofs, status)


def same(got, want):
    return len(got) == len(want) and all(a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))


@pytest.fixture(scope="module")
def S():
    s = System()
    assert PKG.R1cs(s.r1cs).qap_info()["domain_size"] == 8
    # what a fresh set of handles gives for each batch alone; computed once, compared against everywhere
    s.want = {}
    for lo, hi in BATCHES:
        hs = s.handles()
        s.want[lo, hi] = run_device(s, hs, lo, hi)
        for h in hs:
            h.close()
    first = np.concatenate([s.want[b][0] for b in BATCHES])
    assert (first >= 0).nonzero()[0].tolist() == [4]  # the planted fault and nothing else
    status = np.concatenate([s.want[b][5] for b in BATCHES])
    assert status.tolist() == [PKG.VERIFY_VALID] * 4 + [PKG.VERIFY_EQUATION] + [PKG.VERIFY_VALID] * 3
    return s


# -- workspace growth and reuse ---------------------------------------------------------------------------------------------------
def test_one_handle_across_batches_1_5_2_equals_fresh_handles(S):
    hs = S.handles()
    for lo, hi in BATCHES:  # grows at 5, is reused at 2
        assert same(run_device(S, hs, lo, hi), S.want[lo, hi]), (lo, hi)


def test_one_handle_across_batches_under_a_small_cap(S, tmp_path):
    """CWC_R1CS_QAP_WORKSPACE_MB and CWC_GROTH16_WORKSPACE_MB are read once per process: a child process with 1 MiB caps"""
    np.save(tmp_path / "rows.npy", S.rows)
    np.save(tmp_path / "rs.npy", S.rs)
    (tmp_path / "c.r1cs").write_bytes(S.r1cs)
    (tmp_path / "c.zkey").write_bytes(S.zkey)
    code = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
import cwc_import
import torch
P = cwc_import.load()
d = %r
rows, rs = np.load(d + "/rows.npy"), np.load(d + "/rs.npy")
zkey = open(d + "/c.zkey", "rb").read()
r, g, vk = P.R1cs(open(d + "/c.r1cs", "rb").read()), P.Groth16(zkey), P.Groth16VerifyingKey.from_zkey(zkey)
for lo, hi in %r:
    w = torch.from_numpy(rows[lo:hi]).cuda()
    first, nfail = r.check_batch_device(w)
    h_r, h_z = r.qap_batch_device(w), g.qap_batch_device(w)
    proofs = g.prove_batch_device(w, rs=rs[lo:hi])
    status = vk.verify_batch_device(proofs, torch.from_numpy(np.ascontiguousarray(rows[lo:hi, 1:1 + %d])).cuda())
    torch.cuda.synchronize()
    np.savez(d + "/out_%%d_%%d.npz" %% (lo, hi), *[t.cpu().numpy() for t in (first, nfail, h_r, h_z, proofs, status)])
""" % (ROOT, str(tmp_path), BATCHES, N_PUB)
    env = dict(os.environ, CWC_R1CS_QAP_WORKSPACE_MB="1", CWC_GROTH16_WORKSPACE_MB="1")
    subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=300)
    for lo, hi in BATCHES:
        z = np.load(tmp_path / ("out_%d_%d.npz" % (lo, hi)))
        assert same([z["arr_%d" % i] for i in range(6)], S.want[lo, hi]), (lo, hi)


# -- phase timers ---------------------------------------------------------------------------------------------------------------
def _timed_ok(ms, keys):
    return set(ms) == set(keys) and all(math.isfinite(v) and v >= 0 for v in ms.values())


def test_phase_timers_on_report_off(S):
    r, g, vk = S.handles()
    lo, hi = BATCHES[2]
    with pytest.raises(PKG.WitnessCalcError, match="no QAP phase times"):
        r.qap_phase_ms()
    with pytest.raises(PKG.WitnessCalcError, match="no prover phase times"):
        g.phase_ms()
    for on in (r.qap_time_phases, g.time_phases):
        on()
        on(True)  # twice in a row
    assert same(run_device(S, (r, g, vk), lo, hi), S.want[lo, hi])
    ms = r.qap_phase_ms()
    assert _timed_ok(ms, QAP_PHASES), ms
    ms = g.phase_ms()
    assert _timed_ok(ms, PKG.GROTH16_PHASES), ms
    r.qap_time_phases(False)
    g.time_phases(False)
    with pytest.raises(PKG.WitnessCalcError, match="no QAP phase times"):
        r.qap_phase_ms()
    with pytest.raises(PKG.WitnessCalcError, match="no prover phase times"):
        g.phase_ms()
    assert same(run_device(S, (r, g, vk), lo, hi), S.want[lo, hi])
    r.qap_time_phases(False)  # off while off
    g.time_phases(False)


def test_closing_handles_with_timers_on_or_never_used(S):
    lo, hi = BATCHES[0]
    r, g, vk = S.handles()
    r.qap_time_phases()
    g.time_phases()
    assert same(run_device(S, (r, g, vk), lo, hi), S.want[lo, hi])
    r2, g2, vk2 = S.handles()  # their timers are never touched
    assert same(run_device(S, (r2, g2, vk2), lo, hi), S.want[lo, hi])
    r3, g3, _ = S.handles()  # timers on, no call
    r3.qap_time_phases()
    g3.time_phases()
    for h in (g, r, vk, r2, g2, vk2, g3, r3):
        h.close()


# -- error, then reuse ----------------------------------------------------------------------------------------------------------
def test_a_refused_call_leaves_the_handle_as_it_was(S):
    hs = r, g, vk = S.handles()
    lo, hi = BATCHES[2]
    assert same(run_device(S, hs, lo, hi), S.want[lo, hi])
    wide = np.zeros((2, S.pl.n_wires + 1, 32), dtype=np.uint8)
    for call in (r.check_batch_device, r.qap_batch_device):
        with pytest.raises(PKG.WitnessCalcError, match="elements, the circuit"):
            call(_cuda(wide))
    with pytest.raises(PKG.WitnessCalcError, match="elements, the circuit"):
        r.qap_batch(wide)
    with pytest.raises(PKG.WitnessCalcError, match="elements, the key nVars"):
        g.qap_batch_device(_cuda(wide))
    with pytest.raises(PKG.WitnessCalcError, match="elements, the zkey nVars"):
        g.prove_batch_device(_cuda(wide), rs=S.rs[lo:hi])
    with pytest.raises(PKG.WitnessCalcError, match="elements, the zkey nVars"):
        g.prove_batch(wide, rs=S.rs[lo:hi])
    with pytest.raises(PKG.WitnessCalcError, match=r"rs\[1\]\[0\] is not below r"):
        g.prove_batch_device(_cuda(S.rows[lo:hi]), rs=[(1, 2), (R, 3)])
    with pytest.raises(PKG.WitnessCalcError, match="public signals per row"):
        _verify_wrong_width(vk, S, lo, hi)
    assert same(run_device(S, hs, lo, hi), S.want[lo, hi])


def _verify_wrong_width(vk, S, lo, hi):
    """the verifier's host entry point with one public signal per row too many (the Python wrapper would refuse it itself)"""
    import ctypes
    proofs = np.ascontiguousarray(S.want[lo, hi][4])
    pub = np.zeros((hi - lo, N_PUB + 1, 32), dtype=np.uint8)
    out = np.zeros(hi - lo, dtype=np.uint32)
    st = PKG.GwStatus()
    rc = PKG.r1cs_lib().gwb_groth16_verify_batch_host(vk._h, proofs.ctypes.data, pub.ctypes.data, N_PUB + 1, hi - lo, out.ctypes.data, ctypes.byref(st))
    PKG._r1cs_check(rc, st)


# -- lifetime -------------------------------------------------------------------------------------------------------------------
def test_three_handles_of_each_kind_interleaved(S):
    sets = [S.handles() for _ in range(3)]
    idle = S.handles()  # never touch the device
    for k, (lo, hi) in enumerate(BATCHES):
        assert same(run_device(S, sets[k], lo, hi), S.want[lo, hi])
    sets[1][0].close()
    sets[1][2].close()
    lo, hi = BATCHES[0]
    assert same(run_device(S, sets[0], lo, hi), S.want[lo, hi])
    sets[1][1].close()
    sets[0][1].close()
    lo, hi = BATCHES[1]
    assert same(run_device(S, sets[2], lo, hi), S.want[lo, hi])
    for hs in sets + [idle]:
        for h in hs:
            h.close()
            h.close()  # a no-op


def test_a_groth16_outlives_its_sibling_on_the_same_r1cs(S):
    r = PKG.R1cs(S.r1cs)
    g1, g2 = PKG.Groth16(S.zkey, r), PKG.Groth16(S.zkey, r)
    lo, hi = BATCHES[1]
    d = _cuda(S.rows[lo:hi])
    want = S.want[lo, hi][4]  # (the witness map of the .r1cs and of the key's section 4 are the same map)
    for g in (g1, g2):
        assert np.array_equal(_host(g.prove_batch_device(d, rs=S.rs[lo:hi]))[0], want)
    g1.close()
    assert np.array_equal(_host(g2.prove_batch_device(d, rs=S.rs[lo:hi]))[0], want)
    assert np.array_equal(_host(r.qap_batch_device(d))[0], S.want[lo, hi][2])
    g2.close()
    assert np.array_equal(_host(r.qap_batch_device(d))[0], S.want[lo, hi][2])
    r.close()


# -- host entry points ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [0, 1, 3])
def test_host_entry_points_agree_with_their_device_twins(S, b):
    hs = r, g, vk = S.handles()
    lo, hi = 3, 3 + b  # (row 4, the failing one, is in the batch of 3)
    rows, rs = S.rows[lo:hi], S.rs[lo:hi]
    first, nfail = r.check_batch(rows)
    proofs = g.prove_batch(rows, rs=rs if b else None)
    host = [first.view(np.int32), nfail.view(np.int32), r.qap_batch(rows), g.qap_batch(rows), proofs,
            vk.verify_batch(proofs, np.ascontiguousarray(S.publics(lo, hi))).view(np.int32)]
    if b == 0:  # nothing was allocated or uploaded: the handles have not chosen a device
        assert [x.shape for x in host] == [(0,), (0,), (0, 8, 32), (0, 8, 32), (0, 256), (0,)]
    d = _cuda(rows)
    dev_first, dev_nfail = r.check_batch_device(d)
    dev_proofs = g.prove_batch_device(d, rs=rs if b else None)
    dev = _host(dev_first, dev_nfail, r.qap_batch_device(d), g.qap_batch_device(d), dev_proofs,
                vk.verify_batch_device(dev_proofs, _cuda(S.publics(lo, hi))))
    assert same(host, dev)
    if b == 3:
        assert host[0].tolist() != [-1, -1, -1] and host[5].tolist() == [PKG.VERIFY_VALID, PKG.VERIFY_EQUATION, PKG.VERIFY_VALID]
    for h in hs:
        h.close()
