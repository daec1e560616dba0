"""The Groth16 verifier and the BN254 pairing (r1cs/verify.hip, include/graph_witness_groth16_verify.h) on an MI355X, against
the plain-Python pairing of tests/bn254_pairing.py (flat Fq12, a different representation from the device's tower): exact GT
bytes of the pairing aid, prover round trips on trapdoor systems, forgeries through the trapdoor (the verifier checks exactly
the equation), every negative status, infinity, nPublic 0 .. 256, batch 0 and 1, every entry point and the CLI, the key from
the zkey and from JSON, vk_alphabeta_12, and witness -> proof -> verification on one stream."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import cwc_import
from tests import bn254_pairing as BP
from tests import groth16_fixtures as GF
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
R, Q = GF.R, GF.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "circom-witnesscalc_amd", "groth16-verify")
VALID, PUBLIC, POINT, SUBGROUP, EQUATION = (PKG.VERIFY_VALID, PKG.VERIFY_PUBLIC, PKG.VERIFY_POINT, PKG.VERIFY_SUBGROUP,
                                            PKG.VERIFY_EQUATION)

pytestmark = pytest.mark.gpu


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _g1b(p):
    return bytes(64) if p is None else p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")


def _g2b(p):
    return bytes(128) if p is None else b"".join(x.to_bytes(32, "little") for x in (p[0][0], p[0][1], p[1][0], p[1][1]))


def _pair_dev(ps, qs):
    import torch
    g1 = np.frombuffer(b"".join(map(_g1b, ps)), dtype=np.uint8).reshape(-1, 64)
    g2 = np.frombuffer(b"".join(map(_g2b, qs)), dtype=np.uint8).reshape(-1, 128)
    out = PKG.bn254_pairing_batch_device(_cuda(g1), _cuda(g2))
    torch.cuda.synchronize()
    return [bytes(r) for r in out.cpu().numpy()]


# -- the pairing aid ------------------------------------------------------------------------------------------------------------
def test_pairing_of_the_generators():
    got = _pair_dev([GF.G1_GEN], [GF.G2_GEN])[0]
    assert got == BP.gt_bytes(BP.pairing(GF.G1_GEN, GF.G2_GEN))


def test_pairing_batch_bilinear():
    rnd = random.Random(1)
    ab = [(rnd.randrange(1, R), rnd.randrange(1, R)) for _ in range(32)]
    ps = GF.G1.gen_muls([a for a, _ in ab])
    qs = GF.G2.gen_muls([b for _, b in ab])
    got = _pair_dev(ps, qs)
    e = BP.pairing(GF.G1_GEN, GF.G2_GEN)
    for (a, b), g in zip(ab, got):
        assert g == BP.gt_bytes(BP.power(e, a * b % R))


def test_pairing_infinity_gives_one():
    got = _pair_dev([None, GF.G1_GEN, None], [GF.G2_GEN, None, None])
    assert got == [BP.gt_bytes(BP.ONE)] * 3


# -- keys with known logs -------------------------------------------------------------------------------------------------------
class Key:
    """A verifying key with known logs alpha, beta, gamma, delta, ic_i; forged proofs through the trapdoor.  The logs are random
    unless chosen (ic: {index: log}); a log 0 is the point at infinity."""

    def __init__(self, n_public, seed, alpha=None, beta=None, gamma=None, delta=None, ic=None):
        rnd = self.rnd = random.Random(seed)
        self.n = n_public
        drawn = [rnd.randrange(1, R) for _ in range(4)]
        self.alpha, self.beta, self.gamma, self.delta = (d if c is None else c % R for d, c in zip(drawn, (alpha, beta, gamma, delta)))
        self.ic = [rnd.randrange(1, R) for _ in range(n_public + 1)]
        for i, log in (ic or {}).items():
            self.ic[i] = log % R
        g1 = GF.G1.gen_muls([self.alpha] + self.ic)
        g2 = GF.G2.gen_muls([self.beta, self.gamma, self.delta])
        self.points = _g1b(g1[0]) + b"".join(map(_g2b, g2)) + b"".join(map(_g1b, g1[1:]))
        self.vk = PKG.Groth16VerifyingKey(self.points, n_public)

    def ic_log(self, pub):
        return (self.ic[0] + sum(s * k for s, k in zip(pub, self.ic[1:]))) % R

    def holds(self, a, b, c, pub):
        """the verifier's equation in the logs: a b = alpha beta + gamma ic(pub) + delta c (mod r)"""
        return (a * b - self.alpha * self.beta - self.gamma * self.ic_log(pub) - self.delta * c) % R == 0

    def c_for(self, a, b, pub):
        return (a * b - self.alpha * self.beta - self.gamma * self.ic_log(pub)) * pow(self.delta, -1, R) % R

    def forge(self, pubs, a=None, b=None, c=None):
        """[(a, b, c)] logs of valid proofs for the given signals (c computed unless given)"""
        out = []
        for pub in pubs:
            a_ = self.rnd.randrange(1, R) if a is None else a
            b_ = self.rnd.randrange(1, R) if b is None else b
            out.append((a_, b_, self.c_for(a_, b_, pub) if c is None else c))
        return out


def _proof_rows(logs):
    p1 = GF.G1.gen_muls([x for a, _, c in logs for x in (a, c)])
    p2 = GF.G2.gen_muls([b for _, b, _ in logs])
    return np.frombuffer(b"".join(GF.proof_bytes(p1[2 * i], p2[i], p1[2 * i + 1]) for i in range(len(logs))),
                         dtype=np.uint8).reshape(len(logs), 256).copy()


def _signals(rnd, n, b):
    return [[rnd.randrange(R) for _ in range(n)] for _ in range(b)]


def _verify_both(key, proofs, pubs):
    import torch
    host = key.vk.verify_batch(proofs, pubs)
    pa = PKG._public_array(pubs, len(pubs), key.n) if len(pubs) else np.zeros((0, key.n, 32), np.uint8)
    dev = key.vk.verify_batch_device(_cuda(proofs.reshape(-1, 256)), _cuda(pa))
    torch.cuda.synchronize()
    assert np.array_equal(host, dev.cpu().numpy().astype(np.uint32))
    return host


def test_forgeries_through_the_trapdoor():
    key = Key(3, 10)
    pubs = _signals(key.rnd, 3, 6)
    logs = key.forge(pubs)
    assert list(_verify_both(key, _proof_rows(logs), pubs)) == [VALID] * 6
    bad = [(a, b, key.rnd.randrange(R)) for a, b, _ in logs]
    assert list(_verify_both(key, _proof_rows(bad), pubs)) == [EQUATION] * 6


@pytest.mark.parametrize("n_public", [0, 1, 3, 256])
def test_sizes(n_public):
    key = Key(n_public, 20 + n_public)
    b = 2 if n_public == 256 else 5
    pubs = _signals(key.rnd, n_public, b)
    if n_public:
        pubs[0] = [R - 1] * n_public  # the largest signals
        pubs[1] = [0] * n_public
    logs = key.forge(pubs)
    rows = _proof_rows(logs)
    assert list(_verify_both(key, rows, pubs)) == [VALID] * b
    if n_public:
        wrong = [list(p) for p in pubs]
        wrong[-1][-1] = (wrong[-1][-1] + 1) % R
        assert list(_verify_both(key, rows, wrong)) == [VALID] * (b - 1) + [EQUATION]


def test_batch_zero_and_one():
    key = Key(2, 30)
    assert key.vk.verify_batch(np.zeros((0, 256), np.uint8), []).shape == (0,)
    import torch
    d = key.vk.verify_batch_device(_cuda(np.zeros((0, 256), np.uint8)), _cuda(np.zeros((0, 2, 32), np.uint8)))
    torch.cuda.synchronize()
    assert d.shape == (0,)
    pubs = _signals(key.rnd, 2, 1)
    assert list(_verify_both(key, _proof_rows(key.forge(pubs)), pubs)) == [VALID]


def test_negative_rows_and_mixed_batch():
    key = Key(2, 40)
    rnd = key.rnd
    pubs = _signals(rnd, 2, 19)
    rows = _proof_rows(key.forge(pubs))
    want = [VALID] * 19
    # 0: a public signal + 1 -> EQUATION
    pubs[0] = [(pubs[0][0] + 1) % R, pubs[0][1]]
    want[0] = EQUATION
    # 1: a signal >= r -> PUBLIC (even with a bad point as well: the first rule wins)
    pubs[1] = [pubs[1][0], pubs[1][1] + R]
    rows[1, 0] ^= 1
    want[1] = PUBLIC
    # 2: a coordinate >= q (A.x + q keeps the residue) -> POINT
    ax = int.from_bytes(bytes(rows[2, :32]), "little") + Q
    rows[2, :32] = np.frombuffer(ax.to_bytes(32, "little"), np.uint8)
    want[2] = POINT
    # 3, 4, 5: off-curve A, B, C -> POINT
    for i, off in ((3, 32), (4, 128), (5, 224)):
        v = (int.from_bytes(bytes(rows[i, off:off + 32]), "little") + 1) % Q
        rows[i, off:off + 32] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
        want[i] = POINT
    # 6: B on the twist, outside the order-r subgroup -> SUBGROUP
    rows[6, 64:192] = np.frombuffer(_g2b(BP.twist_point_outside_subgroup(random.Random(5))), np.uint8)
    want[6] = SUBGROUP
    # 7, 8, 9: A, B, C at infinity, still valid (a = 0, b = 0, c = 0 through the trapdoor)
    for i, kw in ((7, {"a": 0}), (8, {"b": 0})):
        rows[i] = _proof_rows(key.forge([pubs[i]], **kw))[0]
    a = rnd.randrange(1, R)
    rows[9] = _proof_rows([(a, (key.alpha * key.beta + key.gamma * key.ic_log(pubs[9])) * pow(a, -1, R) % R, 0)])[0]
    assert not rows[7, :64].any() and not rows[8, 64:192].any() and not rows[9, 192:].any()
    # 10: A at infinity with a c that does not fit -> EQUATION; 11 stays valid
    rows[10] = _proof_rows([(0, rnd.randrange(1, R), rnd.randrange(R))])[0]
    want[10] = EQUATION
    # 12 .. 18: as row 2, in each of the other seven coordinate slots (A.y, B's four, C's two) -> POINT
    for i, off in enumerate(range(32, 256, 32), 12):
        v = int.from_bytes(bytes(rows[i, off:off + 32]), "little") + Q
        rows[i, off:off + 32] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
        want[i] = POINT
    assert list(_verify_both(key, rows, pubs)) == want


def test_alphabeta_and_json_round_trip():
    key = Key(2, 50)
    ab = key.vk.alphabeta()
    assert ab == BP.gt_bytes(BP.power(BP.pairing(GF.G1_GEN, GF.G2_GEN), key.alpha * key.beta % R))
    js = key.vk.to_json()
    assert js["protocol"] == "groth16" and js["curve"] == "bn128" and js["nPublic"] == 2 and len(js["IC"]) == 3
    assert js["vk_alpha_1"][2] == "1" and js["vk_beta_2"][2] == ["1", "0"]
    again = PKG.Groth16VerifyingKey.from_json(json.loads(json.dumps(js)))
    assert again.points() == key.points and again.alphabeta() == ab


# -- the prover's proofs --------------------------------------------------------------------------------------------------------
def _system(seed, n_constraints, n_pub_out=1, n_pub_in=2):
    rnd = random.Random(seed)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(n_constraints)]
    pl = F.planted_system(rnd, 6, shapes, [1, R - 1, 2, F.MONT_R, None])
    n_pub = n_pub_out + n_pub_in
    r1 = PKG.R1cs(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=n_pub_out, n_pub_in=n_pub_in))
    T = GF.Trapdoor(pl.constraints, pl.n_wires, n_pub, seed=seed)
    return pl, r1, T, PKG.Groth16(T.zkey, r1)


def test_prover_round_trip_and_entry_points(tmp_path):
    pl, r1, T, g = _system(60, 30)
    rnd = random.Random(61)
    rows = [pl.complete(rnd) for _ in range(6)]
    bad = list(rows[5])
    bad[pl.free[0]] = (bad[pl.free[0]] + 1) % R  # unsatisfied: its proof must fail
    rows[5] = bad
    rs = [(rnd.randrange(R), rnd.randrange(R)) for _ in rows]
    vk = g.verifying_key()
    assert vk.n_public == 3
    pubs = [w[1:4] for w in rows]
    for proofs in (g.prove_batch(F.rows_array(rows), rs=rs), g.prove_batch(F.rows_array(rows))):
        st = vk.verify_batch(proofs, pubs)
        want = [T.verifies(w, *T.proof_logs(w, r_, s_)) for w, (r_, s_) in zip(rows, rs)]
        assert want == [True] * 5 + [False]
        assert list(st) == [VALID] * 5 + [EQUATION]
    # the key from the zkey equals the key from its own JSON, and from_zkey(bytes)
    assert PKG.Groth16VerifyingKey.from_json(vk.to_json()).points() == vk.points()
    assert PKG.Groth16VerifyingKey.from_zkey(T.zkey).points() == vk.points()
    # verify(json) and the CLI on the same proof
    proof = PKG.proof_json(proofs[0])
    pub = [str(x) for x in pubs[0]]
    assert vk.verify(proof, pub) and not vk.verify(PKG.proof_json(proofs[5]), [str(x) for x in pubs[5]])
    (tmp_path / "vk.json").write_text(json.dumps(vk.to_json()))
    (tmp_path / "pub.json").write_text(json.dumps(pub))
    (tmp_path / "proof.json").write_text(json.dumps(proof))
    p = subprocess.run([CLI, str(tmp_path / "vk.json"), str(tmp_path / "pub.json"), str(tmp_path / "proof.json")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "OK!", p.stderr
    (tmp_path / "pub.json").write_text(json.dumps([str((pubs[0][0] + 1) % R)] + pub[1:]))
    p = subprocess.run([CLI, str(tmp_path / "vk.json"), str(tmp_path / "pub.json"), str(tmp_path / "proof.json")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 1 and "EQUATION" in p.stdout


def test_end_to_end_on_one_stream():
    """calc_witness_batch_device -> prove_batch_device -> verify_batch_device on the gadget circuit (two public wires) with a
    trapdoor zkey; one row's public wire tampered with before verifying fails alone"""
    import torch
    C = PKG.graphgen.circuits
    with F.gadget_constraints():
        b = C.build_gadgets()
    cons = F.derive_r1cs(b)
    n_w = len(b._witness)
    g = PKG.Graph(b.to_bin())
    r1 = PKG.R1cs(F.write_r1cs(n_w, cons, n_pub_out=2))
    T = GF.Trapdoor(cons, n_w, 2, seed=70)
    pr = PKG.Groth16(T.zkey, r1)
    vk = pr.verifying_key()
    from tools.synth import synth_inputs
    batch = 8
    d_in = torch.from_numpy(synth_inputs("field", g.n_inputs, batch, 71)).cuda()
    d_w = torch.empty((batch, g.n_witness, 32), dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(batch, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g.calc_witness_batch_device(d_in, d_w, d_st, stream=s)
        d_p = pr.prove_batch_device(d_w, stream=s)
        d_pub = d_w[:, 1:3, :].contiguous()
        d_v = vk.verify_batch_device(d_p, d_pub, stream=s)
        d_pub2 = d_pub.clone()
        d_pub2[3, 0, 0] ^= 1
        d_v2 = vk.verify_batch_device(d_p, d_pub2, stream=s)
    s.synchronize()
    assert not d_st.cpu().numpy().any()
    assert list(d_v.cpu().numpy()) == [VALID] * batch
    assert list(d_v2.cpu().numpy()) == [VALID] * 3 + [EQUATION] + [VALID] * 4
