"""The Groth16 prover (r1cs/msm.hip, gwb_groth16_*) on an MI355X, compared byte for byte with proofs whose discrete logs are
known: trapdoor zkeys over planted systems (tests/groth16_fixtures.py) at domain powers 1 to 10, batches 0, 1, 3 and 70,
both row forms, rows above r, scalar edges (r - 1, 2^253, all-ones digits, zero private wires, a 95 % {0, 1} witness),
infinity and duplicate bases, r = s = 0, pi_A at infinity, an unsatisfied witness, sub-batches under a small workspace cap,
drawn randomness, every entry point and the CLI on the same rows, the refusals, and a known-log zkey behind the witness
calculator at the authV2-class size."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import cwc_import
from tests import groth16_fixtures as GF
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
R = F.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _system(seed, n_constraints, n_pub_out=1, n_pub_in=2, n_free=6, tweak=None):
    """planted system + its trapdoor zkey -> (planted, R1cs, Trapdoor, Groth16)"""
    rnd = random.Random(seed)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(n_constraints)]
    pl = F.planted_system(rnd, n_free, shapes, [1, R - 1, 2, F.MONT_R, None])
    n_pub = n_pub_out + n_pub_in
    r1 = PKG.R1cs(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=n_pub_out, n_pub_in=n_pub_in))
    T = GF.Trapdoor(pl.constraints, pl.n_wires, n_pub, seed=seed, tweak=tweak)
    return pl, r1, T, PKG.Groth16(T.zkey, r1)


def _want(T, rows, rs):
    return T.want_bytes([T.proof_logs(w, r_, s_) for w, (r_, s_) in zip(rows, rs)])


def _rs(rnd, b):
    return [(rnd.randrange(R), rnd.randrange(R)) for _ in range(b)]


def _device(g, rows_arr, **kw):
    import torch
    out = g.prove_batch_device(torch.from_numpy(rows_arr).cuda(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("p", range(1, 11))
def test_domain_powers(p):
    """n_constraints chosen so the domain is 2^p (nC + nPub + 1 rows), three rows, canonical host rows"""
    n_pub_in = 0 if p <= 2 else 2
    n_pub = n_pub_in + (0 if p <= 2 else 1)
    n_c = (1 << p) - n_pub - 1 - random.Random(p).randrange(0, 1 << (p - 1))
    pl, r1, T, g = _system(100 + p, n_c, n_pub_out=n_pub - n_pub_in, n_pub_in=n_pub_in)
    assert T.n == 1 << p and r1.qap_info()["domain_size"] == T.n
    rnd = random.Random(p)
    rows = [pl.complete(rnd) for _ in range(3)]
    rs = _rs(rnd, 3)
    got = g.prove_batch(F.rows_array(rows), rs=rs)
    assert np.array_equal(got, _want(T, rows, rs))
    for w, (r_, s_) in zip(rows, rs):
        assert T.verifies(w, *T.proof_logs(w, r_, s_))


def test_batches_forms_and_rows_above_r():
    pl, r1, T, g = _system(7, 40)
    rnd = random.Random(8)
    rows = [pl.complete(rnd) for _ in range(70)]
    rs = _rs(rnd, 70)
    want = _want(T, rows, rs)
    assert np.array_equal(g.prove_batch(F.rows_array(rows), rs=rs), want)
    assert np.array_equal(_device(g, F.rows_array(rows), rs=rs), want)
    mont = [[F.to_montgomery(x) for x in w] for w in rows]
    assert np.array_equal(_device(g, F.rows_array(mont), rs=rs, montgomery=True), want)
    # elements >= r are reduced mod r (canonical and Montgomery rows)
    above = [[x + R if x + R < (1 << 256) and i % 3 == 1 else x for i, x in enumerate(w)] for w in rows[:3]]
    assert np.array_equal(_device(g, F.rows_array(above), rs=rs[:3]), want[:3])
    mabove = [[x + R if x + R < (1 << 256) and i % 2 else x for i, x in enumerate(w)] for w in mont[:3]]
    assert np.array_equal(_device(g, F.rows_array(mabove), rs=rs[:3], montgomery=True), want[:3])
    for b in (0, 1, 3):
        got = g.prove_batch(F.rows_array(rows[:b]) if b else np.zeros((0, pl.n_wires, 32), np.uint8), rs=rs[:b] if b else None)
        assert got.shape == (b, 256) and np.array_equal(got, want[:b])


def test_scalar_edges_and_skew():
    """r - 1 and 2^253 free wires, all-ones digits, zero private wires, a 95 % {0, 1} witness; edge r, s"""
    pl, r1, T, g = _system(9, 60, n_free=40)
    rnd = random.Random(10)
    rows = []
    for fixed in ({f: R - 1 for f in pl.free}, {f: 1 << 253 for f in pl.free}, {f: (1 << 253) - 1 for f in pl.free},
                  {f: 0 for f in pl.free}, {f: (1 if rnd.random() < 0.5 else 0) if rnd.random() < 0.95 else rnd.randrange(R) for f in pl.free}):
        rows.append(pl.complete(rnd, fixed))
    # a row that is not satisfied but whose private wires are all zero: h and the MSMs still follow the formula
    zero = [1] + [0] * (pl.n_wires - 1)
    rows.append(zero)
    rs = [(R - 1, R - 1), (1 << 253, 1), ((1 << 253) - 1, 2), (0, 0), (1, R - 1), (5, 7)]
    assert np.array_equal(g.prove_batch(F.rows_array(rows), rs=rs), _want(T, rows, rs))


def _dup_inf(logs):
    """infinity bases (A_i, B1_i = O for some wires; H_0 = O) and duplicate bases (wire 5's A, B1 and B2 equal wire 4's)"""
    for key in ("a", "b1", "b2"):
        logs[key][3] = 0
        logs[key][5] = logs[key][4]
    logs["a"][6] = 0
    logs["h"][0] = 0
    logs["c"][1] = logs["c"][0]


def test_infinity_and_duplicate_bases():
    pl, r1, T, g = _system(12, 30, tweak=_dup_inf)
    rnd = random.Random(13)
    rows = [pl.complete(rnd) for _ in range(4)]
    rows[1][4], rows[1][5] = 3, R - 3  # equal bases with opposite scalars: P + (-P)
    rows[2][4], rows[2][5] = 5, 5      # equal bases with equal scalars: a doubling inside a bucket
    rs = _rs(rnd, 4)
    assert np.array_equal(g.prove_batch(F.rows_array(rows), rs=rs), _want(T, rows, rs))


def test_pi_a_at_infinity_and_unsatisfied_witness():
    pl, r1, T, g = _system(14, 25)
    rnd = random.Random(15)
    w = pl.complete(rnd)
    a0 = (T.alpha + sum(x * y for x, y in zip(w, T.logs["a"]))) % R
    r_ = -a0 * pow(T.delta, -1, R) % R  # a = 0: pi_A = O and s pi_A = O inside pi_C
    s_ = rnd.randrange(R)
    assert T.proof_logs(w, r_, s_)[0] == 0
    got = g.prove_batch(F.rows_array([w]), rs=[(r_, s_)])
    assert not got[0, :64].any()
    assert np.array_equal(got, _want(T, [w], [(r_, s_)]))
    bad = list(w)
    bad[pl.free[0]] = (bad[pl.free[0]] + 1) % R
    assert F.check(pl.constraints, bad)[1]
    rs = [(rnd.randrange(R), rnd.randrange(R))]
    assert np.array_equal(g.prove_batch(F.rows_array([bad]), rs=rs), _want(T, [bad], rs))
    assert not T.verifies(bad, *T.proof_logs(bad, *rs[0]))


def test_drawn_randomness():
    pl, r1, T, g = _system(16, 20)
    rnd = random.Random(17)
    rows = F.rows_array([pl.complete(rnd) for _ in range(2)])
    p1, p2 = g.prove_batch(rows), g.prove_batch(rows)
    assert not np.array_equal(p1, p2)
    for pr in (p1, p2):
        for row in pr:
            b = bytes(row)
            v = [int.from_bytes(b[32 * k:32 * k + 32], "little") for k in range(8)]
            assert GF.G1.on_curve((v[0], v[1])) and GF.G1.on_curve((v[6], v[7]))
            assert GF.G2.on_curve(((v[2], v[3]), (v[4], v[5])))


def test_sub_batches_under_a_small_cap(tmp_path):
    """CWC_GROTH16_WORKSPACE_MB is read once per process: a child process with a 1 MiB cap proves 9 rows in sub-batches"""
    pl, r1, T, g = _system(18, 30)
    rnd = random.Random(19)
    rows = [pl.complete(rnd) for _ in range(9)]
    rs = _rs(rnd, 9)
    (tmp_path / "c.r1cs").write_bytes(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=2))
    (tmp_path / "c.zkey").write_bytes(T.zkey)
    np.save(tmp_path / "rows.npy", F.rows_array(rows))
    (tmp_path / "rs.json").write_text(json.dumps([[str(a), str(b)] for a, b in rs]))
    code = ("import sys, json, numpy as np; sys.path.insert(0, %r); import cwc_import; P = cwc_import.load(); d = %r\n"
            "r = P.R1cs(open(d + '/c.r1cs', 'rb').read()); g = P.Groth16(open(d + '/c.zkey', 'rb').read(), r)\n"
            "rs = [(int(a), int(b)) for a, b in json.load(open(d + '/rs.json'))]\n"
            "np.save(d + '/out.npy', g.prove_batch(np.load(d + '/rows.npy'), rs=rs))\n") % (ROOT, str(tmp_path))
    env = dict(os.environ, CWC_GROTH16_WORKSPACE_MB="1")
    subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=300)
    assert np.array_equal(np.load(tmp_path / "out.npy"), _want(T, rows, rs))


def test_entry_points_agree(tmp_path):
    """host, device, .wtns and the CLI on the same row; proof.json / public.json in snarkjs's shape"""
    pl, r1, T, g = _system(20, 35)
    rnd = random.Random(21)
    w = pl.complete(rnd)
    rs = [(rnd.randrange(R), rnd.randrange(R))]
    want = _want(T, [w], rs)
    arr = F.rows_array([w])
    assert np.array_equal(g.prove_batch(arr, rs=rs), want)
    assert np.array_equal(_device(g, arr, rs=rs), want)
    img = b"wtns" + (2).to_bytes(4, "little") + (2).to_bytes(4, "little")
    img += (1).to_bytes(4, "little") + (40).to_bytes(8, "little") + (32).to_bytes(4, "little") + R.to_bytes(32, "little")
    img += pl.n_wires.to_bytes(4, "little")
    img += (2).to_bytes(4, "little") + (32 * pl.n_wires).to_bytes(8, "little") + b"".join(x.to_bytes(32, "little") for x in w)
    proof, public = g.prove_wtns(img, rs=rs)
    assert proof == PKG.proof_json(want[0])
    assert public == [str(x) for x in w[1:T.n_pub + 1]]
    assert proof["protocol"] == "groth16" and proof["curve"] == "bn128" and proof["pi_a"][2] == "1"
    assert len(proof["pi_b"]) == 3 and proof["pi_b"][2] == ["1", "0"]
    # the CLI draws r, s itself: its proof verifies against the points it wrote
    for name, data in (("c.r1cs", F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=2)), ("c.zkey", T.zkey), ("w.wtns", img)):
        (tmp_path / name).write_bytes(data)
    cli = os.path.join(ROOT, "circom-witnesscalc_amd", "groth16-prove")
    subprocess.run([cli, str(tmp_path / "c.r1cs"), str(tmp_path / "c.zkey"), str(tmp_path / "w.wtns"), str(tmp_path / "p.json"),
                    str(tmp_path / "pub.json")], check=True, timeout=300)
    pj = json.loads((tmp_path / "p.json").read_text())
    assert json.loads((tmp_path / "pub.json").read_text()) == public
    assert set(pj) == set(proof) and pj["protocol"] == "groth16" and pj["curve"] == "bn128"
    a = (int(pj["pi_a"][0]), int(pj["pi_a"][1]))
    assert GF.G1.on_curve(a) and GF.G2.on_curve(tuple((int(x), int(y)) for x, y in pj["pi_b"][:2]))
    assert pj != proof  # fresh randomness


def test_refusals():
    pl, r1, T, g = _system(22, 10)
    rnd = random.Random(23)
    w = pl.complete(rnd)
    with pytest.raises(PKG.WitnessCalcError, match="not below r"):
        g.prove_batch(F.rows_array([w]), rs=[(R, 1)])
    with pytest.raises(PKG.WitnessCalcError):
        g.prove_batch(F.rows_array([w[:-1]]), rs=[(1, 1)])
    # the same zkey against systems of another shape
    other = PKG.R1cs(F.write_r1cs(pl.n_wires + 1, pl.constraints, n_pub_out=1, n_pub_in=2))
    with pytest.raises(PKG.WitnessCalcError, match="nVars"):
        PKG.Groth16(T.zkey, other).prove_batch(F.rows_array([w + [0]]), rs=[(1, 1)])
    other = PKG.R1cs(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=1))
    with pytest.raises(PKG.WitnessCalcError, match="nPublic"):
        PKG.Groth16(T.zkey, other).prove_batch(F.rows_array([w]), rs=[(1, 1)])
    more = pl.constraints + [([(0, 1)], [(0, 1)], [(0, 1)])] * T.n
    other = PKG.R1cs(F.write_r1cs(pl.n_wires, more, n_pub_out=1, n_pub_in=2))
    with pytest.raises(PKG.WitnessCalcError, match="domainSize"):
        PKG.Groth16(T.zkey, other).prove_batch(F.rows_array([w]), rs=[(1, 1)])


def test_authv2_class_known_log_chain():
    """calc_witness_batch_device -> prove_batch_device on one stream at the authV2-class size (2^17 domain), against a
    known-log zkey; h from R1cs.qap_batch (pinned exactly by test_gpu_r1cs_qap.py)"""
    import torch
    C = PKG.graphgen.circuits
    with F.gadget_constraints():
        b = C.build_authv2_class()
    cons = F.derive_r1cs(b)
    g = PKG.Graph(b.to_bin())
    r1 = PKG.R1cs(F.write_r1cs(len(b._witness), cons))
    n = r1.qap_info()["domain_size"]
    K = GF.KnownLog(r1.info["n_wires"], 0, n)
    pr = PKG.Groth16(K.zkey, r1)
    from tools.synth import synth_inputs
    batch = 3
    rnd = random.Random(24)
    rs = _rs(rnd, batch)
    d_in = torch.from_numpy(synth_inputs("field", g.n_inputs, batch, 43)).cuda()
    d_w = torch.empty((batch, g.n_witness, 32), dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(batch, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g.calc_witness_batch_device(d_in, d_w, d_st, stream=s)
        d_p = pr.prove_batch_device(d_w, stream=s, rs=rs)
    s.synchronize()
    assert not d_st.cpu().numpy().any()
    rows = d_w.cpu().numpy()
    hs = r1.qap_batch(rows)
    logs = []
    for i in range(batch):
        w = F.row_ints(rows[i])
        h = [int.from_bytes(bytes(x), "little") for x in hs[i]]
        logs.append(K.proof_logs(w, h, *rs[i]))
    p1 = GF.G1.gen_muls([x for a, _, c in logs for x in (a, c)])
    p2 = GF.G2.gen_muls([b_ for _, b_, _ in logs])
    want = np.frombuffer(b"".join(GF.proof_bytes(p1[2 * i], p2[i], p1[2 * i + 1]) for i in range(batch)), dtype=np.uint8).reshape(batch, 256)
    assert np.array_equal(d_p.cpu().numpy(), want)
