"""The Groth16 witness map (r1cs/qap.hip, gwb_r1cs_qap_*) on an MI355X, compared exactly with the plain-Python restatement
(tests/qap_reference.py): planted systems with public signals at every domain power through 2^13 (the in-LDS sizes and the
first four-step sizes), a 2^17 domain on sampled points, every tile width, both row and output forms, rows above r,
unsatisfied witnesses, batches 0 and 1, a system without constraints, sub-batches under a small workspace cap, every entry
point on the same rows, the refusals, and the whole chain behind the witness calculator on the authV2-class graph."""
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

import cwc_import
from tests import qap_reference as Q
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
R = F.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_WIDTHS = (1, 2, 4, 8, 16, 32, 64, 0)
POOL = [1, R - 1, 2, F.MONT_R, None]

pytestmark = pytest.mark.gpu


def _system(rnd, n_constraints, n_pub_out=1, n_pub_in=2, n_free=6):
    """a planted system of n_constraints constraints with public signals; -> (planted, r1cs bytes, n_pub)"""
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(n_constraints)]
    pl = F.planted_system(rnd, n_free, shapes, POOL)
    n_pub = n_pub_out + n_pub_in
    assert 1 + n_pub <= pl.n_wires
    data = F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=n_pub_out, n_pub_in=n_pub_in, n_prv_in=0)
    return pl, data, n_pub


def _want(cons, n_pub, rows, montgomery=False):
    """[B, n, 32] canonical h of each row (rows of ints; Montgomery-form rows are converted first)"""
    out = []
    for row in rows:
        w = [F.from_montgomery(x % R) for x in row] if montgomery else row
        out.append(Q.h_bytes(Q.h_of(cons, n_pub, w)))
    return np.stack(out) if out else None


def _mont_bytes(h):
    """canonical h uint8 [.., 32] -> Montgomery form"""
    flat = h.reshape(-1, 32)
    return np.stack([np.frombuffer(F.to_montgomery(int.from_bytes(bytes(x), "little")).to_bytes(32, "little"), dtype=np.uint8)
                     for x in flat]).reshape(h.shape)


def _device(r, arr, **kw):
    import torch
    h = r.qap_batch_device(torch.from_numpy(arr).cuda(), **kw)
    torch.cuda.synchronize()
    return h.cpu().numpy()


def _assert_h(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=-1).reshape(-1))
    assert bad.size == 0, "%s: %d of %d elements differ, first (row, j) %s" % (
        what, bad.size, got.shape[0] * got.shape[1], [divmod(int(k), got.shape[1]) for k in bad[:6]])


def _wtns(row):
    """a .wtns v2 image of one row (ints below r)"""
    hdr = struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<I", len(row))
    vals = b"".join(x.to_bytes(32, "little") for x in row)
    return b"wtns" + struct.pack("<II", 2, 2) + struct.pack("<IQ", 1, len(hdr)) + hdr + struct.pack("<IQ", 2, len(vals)) + vals


@pytest.mark.parametrize("p", range(1, 14))
def test_planted_domain_powers(pkg, p):
    """N = nC + nPub + 1 lands in (2^(p-1), 2^p]; rows satisfied and unsatisfied; host and device paths"""
    rnd = random.Random(100 + p)
    n_pub_out, n_pub_in = (0, 0) if p == 1 else (1, 2)
    lo = (1 << (p - 1)) + 1 if p > 1 else 1
    n_rows = rnd.randrange(lo, (1 << p) + 1) if p > 3 else (1 << p)
    n_c = max(0, n_rows - n_pub_out - n_pub_in - 1)
    pl, data, n_pub = _system(rnd, n_c, n_pub_out, n_pub_in)
    r = PKG.R1cs(data)
    info = r.qap_info()
    assert info["domain_power"] == p and info["n_rows"] == n_c + n_pub + 1
    rows = [pl.complete(rnd) for _ in range(3)]
    rows[1][rnd.randrange(1, pl.n_wires)] = rnd.randrange(R)  # unsatisfied: h still matches (c = a o b)
    want = _want(pl.constraints, n_pub, rows)
    arr = F.rows_array(rows)
    _assert_h(r.qap_batch(arr), want, "host p=%d" % p)
    _assert_h(_device(r, arr), want, "device p=%d" % p)


@pytest.mark.parametrize("p", (4, 11, 12))
def test_tile_widths_and_forms(pkg, p):
    """every tile width of the evaluation kernel; canonical and Montgomery rows in, canonical and Montgomery h out"""
    rnd = random.Random(200 + p)
    pl, data, n_pub = _system(rnd, (1 << p) - 4 - rnd.randrange(0, 1 << (p - 2)))
    r = PKG.R1cs(data)
    rows = [pl.complete(rnd) for _ in range(5)]
    want = _want(pl.constraints, n_pub, rows)
    want_m = _mont_bytes(want)
    canon = F.rows_array(rows)
    mont = F.rows_array([[F.to_montgomery(x) for x in row] for row in rows])
    for t in TILE_WIDTHS:
        r.set_tile_width(t)
        _assert_h(_device(r, canon), want, "t=%d canonical" % t)
        _assert_h(_device(r, mont, montgomery=True), want, "t=%d montgomery in" % t)
    r.set_tile_width(0)
    _assert_h(_device(r, canon, montgomery_out=True), want_m, "montgomery out")
    _assert_h(_device(r, mont, montgomery=True, montgomery_out=True), want_m, "montgomery in and out")
    _assert_h(r.qap_batch(canon, montgomery_out=True), want_m, "host montgomery out")


def test_rows_above_r(pkg):
    """elements >= r (also in the public wires the input rows read) are reduced, in both row forms"""
    rnd = random.Random(300)
    pl, data, n_pub = _system(rnd, 200, 2, 3)
    r = PKG.R1cs(data)
    rows = [pl.complete(rnd) for _ in range(4)]
    big = [[x + R if x + R < (1 << 256) and rnd.random() < 0.5 else x for x in row] for row in rows]
    for row in big:
        row[1] = row[1] % R + R  # a public wire, read directly by an input row
    want = _want(pl.constraints, n_pub, [[x % R for x in row] for row in big])
    _assert_h(_device(r, F.rows_array(big)), want, "canonical rows above r")
    _assert_h(r.qap_batch(F.rows_array(big)), want, "host rows above r")
    mont_big = [[F.to_montgomery(x % R) + (R if rnd.random() < 0.5 else 0) for x in row] for row in big]
    mont_big = [[x if x < (1 << 256) else x - R for x in row] for row in mont_big]
    _assert_h(_device(r, F.rows_array(mont_big), montgomery=True), want, "montgomery rows above r")


def test_batch_zero_and_one(pkg):
    import torch
    rnd = random.Random(400)
    pl, data, n_pub = _system(rnd, 40)
    r = PKG.R1cs(data)
    n = r.qap_info()["domain_size"]
    empty = np.zeros((0, pl.n_wires, 32), dtype=np.uint8)
    assert r.qap_batch(empty).shape == (0, n, 32)
    assert tuple(r.qap_batch_device(torch.from_numpy(empty).cuda()).shape) == (0, n, 32)
    rows = [pl.complete(rnd)]
    _assert_h(_device(r, F.rows_array(rows)), _want(pl.constraints, n_pub, rows), "batch 1")


def test_no_constraints(pkg):
    """an `.r1cs` without constraints: the evaluation launch is skipped (its clamp to the last row has no row to clamp to), the
    input rows come from the witness, b is zero at every point, so h = A B - C is zero whatever the row holds"""
    rnd = random.Random(450)
    n_wires = 7  # wire 0, one public output, one public input, four free wires
    r = PKG.R1cs(F.write_r1cs(n_wires, [], n_pub_out=1, n_pub_in=1, n_prv_in=0))
    info = r.qap_info()
    assert info["n_rows"] == 3 and info["domain_size"] == 4, info
    rows = [[1] + [rnd.randrange(R) for _ in range(n_wires - 1)] for _ in range(3)]
    want = _want([], 2, rows)
    assert want.shape == (3, 4, 32) and not want.any()
    canon = F.rows_array(rows)
    mont = F.rows_array([[F.to_montgomery(x) for x in row] for row in rows])
    for out in (False, True):  # (zero is zero in both forms)
        _assert_h(r.qap_batch(canon, montgomery_out=out), want, "host, montgomery_out=%s" % out)
        for t in (0, 64):
            r.set_tile_width(t)
            _assert_h(_device(r, canon, montgomery_out=out), want, "t=%d canonical, montgomery_out=%s" % (t, out))
            _assert_h(_device(r, mont, montgomery=True, montgomery_out=out), want, "t=%d montgomery in, montgomery_out=%s" % (t, out))


def test_sub_batches_under_a_small_cap(pkg):
    """CWC_R1CS_QAP_WORKSPACE_MB = 1 at a 2^13 domain (512 KiB per row): sub-batches of two rows, in a child process"""
    code = r"""
import random, sys
import numpy as np
sys.path.insert(0, %r)
import cwc_import
from tests import r1cs_fixtures as F, qap_reference as Q
import torch
PKG = cwc_import.load()
rnd = random.Random(500)
shapes = [{"a": 2, "b": 2, "c": 1} for _ in range(5000)]
pl = F.planted_system(rnd, 5, shapes, [1, None])
r = PKG.R1cs(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=1))
info = r.qap_info()
assert info["domain_power"] == 13 and info["workspace_bytes_per_row"] == 1 << 19, info
rows = [pl.complete(rnd) for _ in range(7)]
rows[3][2] = 12345
h = r.qap_batch_device(torch.from_numpy(F.rows_array(rows)).cuda())
torch.cuda.synchronize()
h = h.cpu().numpy()
for s, row in enumerate(rows):
    want = Q.h_bytes(Q.h_of(pl.constraints, 2, row))
    assert (h[s] == want).all(), s
print("ok")
""" % ROOT
    env = dict(os.environ, CWC_R1CS_QAP_WORKSPACE_MB="1")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_large_domain_sampled(pkg):
    """a 2^17 domain (three passes: two outer, one in LDS) on sampled rows and points, by Lagrange evaluation"""
    rnd = random.Random(600)
    n_w, n_c, n_pub = 300, 70000, 5
    cons = []
    for _ in range(n_c):
        lc = lambda k: {rnd.randrange(n_w): rnd.choice((1, R - 1, rnd.randrange(R))) for _ in range(k)}
        cons.append((lc(rnd.randrange(1, 3)), lc(rnd.randrange(0, 3)), lc(1)))
    r = PKG.R1cs(F.write_r1cs(n_w, cons, n_pub_out=2, n_pub_in=3))
    assert r.qap_info()["domain_power"] == 17
    rows = [[1] + [rnd.randrange(R) for _ in range(n_w - 1)] for _ in range(3)]
    h = _device(r, F.rows_array(rows))
    n = 1 << 17
    js = [0, 1, 2, 4095, 65536, n - 1] + rnd.sample(range(n), 4)
    for s in (0, 2):
        a, b, c = Q.qap_rows(cons, n_pub, rows[s])
        want = Q.h_at(a, b, c, js)
        got = [int.from_bytes(bytes(h[s, j]), "little") for j in js]
        assert got == want, s


def test_entry_points_agree(pkg, tmp_path):
    """host, device, Montgomery device, .wtns and the witness-h CLI on the same rows"""
    rnd = random.Random(700)
    pl, data, n_pub = _system(rnd, 300, 1, 1)
    r = PKG.R1cs(data)
    rows = [pl.complete(rnd) for _ in range(2)]
    rows[1][pl.n_wires - 1] = (rows[1][pl.n_wires - 1] + 1) % R
    want = _want(pl.constraints, n_pub, rows)
    arr = F.rows_array(rows)
    _assert_h(r.qap_batch(arr), want, "host")
    _assert_h(r.qap_batch((arr, None)), want, "host (witness, status) pair")
    _assert_h(_device(r, arr), want, "device")
    _assert_h(_device(r, F.rows_array([[F.to_montgomery(x) for x in row] for row in rows]), montgomery=True), want, "montgomery")
    cli = os.path.join(os.path.dirname(PKG.R1CS_LIB_PATH), "witness-h")
    (tmp_path / "c.r1cs").write_bytes(data)
    for s, row in enumerate(rows):
        img = _wtns(row)
        _assert_h(r.qap_wtns(img)[None], want[s:s + 1], "wtns %d" % s)
        (tmp_path / "w.wtns").write_bytes(img)
        p = subprocess.run([cli, str(tmp_path / "c.r1cs"), str(tmp_path / "w.wtns"), str(tmp_path / "h.bin")], capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        got = np.frombuffer((tmp_path / "h.bin").read_bytes(), dtype=np.uint8).reshape(-1, 32)
        _assert_h(got[None], want[s:s + 1], "cli %d" % s)
    # a .wtns element at r is refused with the check's message
    bad = bytearray(_wtns(rows[0]))
    bad[-32:] = R.to_bytes(32, "little")
    with pytest.raises(PKG.WitnessCalcError, match="is not below r"):
        r.qap_wtns(bytes(bad))


def test_refusals(pkg):
    import torch
    rnd = random.Random(800)
    pl, data, n_pub = _system(rnd, 10)
    r = PKG.R1cs(data)
    short = F.rows_array([pl.complete(rnd)[:-1]])
    with pytest.raises(PKG.WitnessCalcError, match="elements, the circuit"):
        r.qap_batch(short)
    with pytest.raises(PKG.WitnessCalcError, match="elements, the circuit"):
        r.qap_batch_device(torch.from_numpy(short).cuda())
    # 2^27 + 1 rows (N = nPub + 1 with nPub = 2^27): domain 2^28 refused; no constraints, so only the wire map is large
    n_pub = 1 << 27
    n_wires = n_pub + 1
    big = F.container([(1, F.header_section(n_wires, 0, n_pub, 0, n_labels=1, n_constraints=0)), (2, b""),
                       (3, bytes(8 * n_wires))])
    rb = PKG.R1cs(big)
    del big
    with pytest.raises(PKG.WitnessCalcError, match="at most 2.27"):
        rb.qap_info()
    with pytest.raises(PKG.WitnessCalcError, match="at most 2.27"):
        rb.qap_batch(np.zeros((1, 1, 32), dtype=np.uint8))
    rb.close()


def test_authv2_class_chain(pkg):
    """calc_witness_batch_device, then qap_batch_device on the same stream, against qap_batch on the copied-back rows, and
    a sampled row against the restatement"""
    import torch
    C = PKG.graphgen.circuits
    with F.gadget_constraints():
        b = C.build_authv2_class()
    cons = F.derive_r1cs(b)
    g = PKG.Graph(b.to_bin())
    r = PKG.R1cs(F.write_r1cs(len(b._witness), cons))
    assert r.qap_info()["domain_power"] == 17
    from tools.synth import synth_inputs
    batch = 64
    d_in = torch.from_numpy(synth_inputs("field", g.n_inputs, batch, 41)).cuda()
    d_w = torch.empty((batch, g.n_witness, 32), dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(batch, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g.calc_witness_batch_device(d_in, d_w, d_st, stream=s)
        d_h = r.qap_batch_device(d_w, stream=s)
    s.synchronize()
    assert not d_st.cpu().numpy().any()
    rows = d_w.cpu().numpy()
    h_dev = d_h.cpu().numpy()
    _assert_h(r.qap_batch(rows), h_dev, "device chain vs host")
    rnd = random.Random(900)
    row = F.row_ints(rows[5])
    a, b_, c = Q.qap_rows(cons, 0, row)
    js = rnd.sample(range(1 << 17), 3)
    assert [int.from_bytes(bytes(h_dev[5, j]), "little") for j in js] == Q.h_at(a, b_, c, js)
