"""The Groth16 key setup from a powers-of-tau file (r1cs/setup_ptau.hip, gwb_groth16_setup_ptau) on an MI355X.  The oracle is
the existing Python: a `.ptau` written from known (tau, alpha, beta) must give, byte for byte, the key of
tests/groth16_fixtures.py's Trapdoor(tau, alpha, beta, gamma = 1, delta); affine canonical points are unique, so every
comparison is byte equality.  The group inverse DFT against ((1 / N) sum_i w^(-k i) s_i) G at every size from 2 to 2^10 in
both groups, the planted systems of domain powers 1 to 8, the column edges and the skewed column of
test_gpu_groth16_setup.py (constructions copied), delta = 1, r - 1 and a random one, the Lagrange source modes, a drawn delta
through the pairing, the CLI chain, a point fault found on the device, and the phase timer."""
import functools
import json
import math
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import cwc_import
from tests import groth16_fixtures as GF
from tests import ptau_fixtures as PF
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
R, Q = F.R, GF.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "circom-witnesscalc_amd")
NO_CONTRIBUTIONS = bytes(64) + struct.pack("<I", 0)
_rnd = random.Random(300)
TAU, ALPHA, BETA, TAU_OTHER, DELTA_RANDOM = (_rnd.randrange(2, R) for _ in range(5))
DELTAS = {"delta_1": 1, "delta_r_minus_1": R - 1, "delta_random": DELTA_RANDOM}
DELTA1_AT = 84 + 64 + 64 + 128 + 128  # delta1 in section 2

pytestmark = pytest.mark.gpu


def sections(zkey):
    """`.zkey` bytes -> ([section ids in file order], {id: body})"""
    assert zkey[:4] == b"zkey" and struct.unpack_from("<I", zkey, 4)[0] == 1
    n_sec = struct.unpack_from("<I", zkey, 8)[0]
    off, ids, out = 12, [], {}
    for _ in range(n_sec):
        sid, size = struct.unpack_from("<IQ", zkey, off)
        off += 12
        ids.append(sid)
        out[sid] = zkey[off:off + size]
        off += size
    assert off == len(zkey)
    return ids, out


# -- points from the device's fixed-base multiplication (existing code, tested against Curve.gen_muls) --------------------------
def device_canonical(group, scalars):
    """[k] -> uint8 [n, 64 group]: k G, canonical affine, zero bytes for infinity"""
    import torch
    arr = np.frombuffer(b"".join((k % R).to_bytes(32, "little") for k in scalars), dtype=np.uint8).reshape(len(scalars), 32)
    out = PKG.bn254_gen_mul_batch_device(torch.from_numpy(arr.copy()).cuda(), group)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def device_points(group, scalars):
    """ptau_fixtures' `points`: the stored form (Montgomery little-endian) of k G"""
    raw = device_canonical(group, scalars).tobytes()
    return b"".join(GF.lem(int.from_bytes(raw[o:o + 32], "little")) for o in range(0, len(raw), 32))


@functools.lru_cache(maxsize=None)
def ptau_sections(power, prepared=False, lagrange_tau=None):
    return PF.sections(power, TAU, ALPHA, BETA, prepared=prepared, lagrange_tau=lagrange_tau, points=device_points)


@functools.lru_cache(maxsize=None)
def ptau(power, prepared=False, lagrange_tau=None):
    return PF.assemble(ptau_sections(power, prepared, lagrange_tau))


def test_the_device_written_file_is_the_python_file():
    assert ptau(2, True) == PF.write_ptau(2, TAU, ALPHA, BETA, prepared=True)


# -- the group inverse DFT ------------------------------------------------------------------------------------------------------
def _idft_inputs(m):
    """scalar vectors of length 2^m: seeded values with zeros, repeated values and pairs s, r - s planted, among them at i and
    i + N / 2 (the operands of the first butterflies: a doubling, a cancellation, O + P, O + O); a constant vector (every
    stage cancels) and a single nonzero value for the small sizes"""
    rnd = random.Random(310 + m)
    n = 1 << m
    if m == 1:
        s, t = rnd.randrange(1, R), rnd.randrange(1, R)
        return [[s, t], [s, s], [s, R - s], [0, s], [s, 0], [0, 0]]
    v = [rnd.randrange(1, R) for _ in range(n)]
    h = n // 2
    v[h] = v[0]                  # P + P and P - P
    v[h + 1] = R - v[1]          # P + (-P) and P - (-P)
    if m >= 3:
        v[2] = 0                 # O + P
        v[3] = v[h + 3] = 0      # O + O
    if m >= 4:
        v[h - 1] = v[h - 2]      # neighbours
        v[h - 3] = R - v[h - 4]
    out = [v]
    if m <= 5:
        c = rnd.randrange(1, R)
        out.append([c] * n)
        one = [0] * n
        one[rnd.randrange(n)] = c
        out.append(one)
    return out


def _point_bytes(p, words):
    if p is None:
        return bytes(32 * words)
    cs = p if words == 2 else (p[0][0], p[0][1], p[1][0], p[1][1])
    return b"".join(x.to_bytes(32, "little") for x in cs)


@pytest.mark.parametrize("m", range(1, 11))
@pytest.mark.parametrize("group", (1, 2))
def test_point_idft(group, m):
    """sizes 2 to 2^10: one stage; fewer and more than 64 groups per stage (both lane mappings, from 2^7); more than a block"""
    import torch
    curve, words = (GF.G1, 2) if group == 1 else (GF.G2, 4)
    n = 1 << m
    for s in _idft_inputs(m):
        want_logs = PF.lag(m, s)
        if m <= 4:  # the definition, term by term
            wi = pow(PF.QR.roots(m)[0], -1, R)
            assert want_logs == [pow(n, -1, R) * sum(pow(wi, k * i, R) * s[i] for i in range(n)) % R for k in range(n)]
        want = np.frombuffer(b"".join(_point_bytes(p, words) for p in curve.gen_muls(want_logs)), dtype=np.uint8).reshape(n, 32 * words)
        d_in = torch.from_numpy(device_canonical(group, s)).cuda()
        got = PKG.bn254_point_idft_batch_device(d_in, group)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.shape == want.shape
        assert np.array_equal(got, want), "group %d, 2^%d points: rows %s differ" % (group, m, np.nonzero((got != want).any(axis=1))[0][:8])


def test_point_idft_arguments():
    import torch
    d = torch.zeros((4, 64), dtype=torch.uint8, device="cuda")
    assert not PKG.bn254_point_idft_batch_device(d, 1).cpu().numpy().any()  # O everywhere
    with pytest.raises(PKG.WitnessCalcError, match="group"):
        PKG.bn254_point_idft_batch_device(d, 3)
    for rows in (1, 3, 6):
        with pytest.raises(PKG.WitnessCalcError, match="power of two"):
            PKG.bn254_point_idft_batch_device(torch.zeros((rows, 64), dtype=torch.uint8, device="cuda"), 1)


# -- keys -----------------------------------------------------------------------------------------------------------------------
def _power_system(p):
    """the planted system of test_gpu_groth16_setup.py::power_case for the domain 2^p"""
    n_pub_in = 0 if p <= 2 else 2
    n_pub = n_pub_in + (0 if p <= 2 else 1)
    n_c = (1 << p) - n_pub - 1 - random.Random(p).randrange(0, 1 << (p - 1))
    rnd = random.Random(100 + p)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(n_c)]
    pl = F.planted_system(rnd, 6, shapes, [1, R - 1, 2, F.MONT_R, None])
    return pl.constraints, pl.n_wires, n_pub - n_pub_in, n_pub_in, p


def _column_edges_system():
    """test_gpu_groth16_setup.py::test_column_edges, with this file's beta"""
    n_c, n_wires = 10, 9
    rnd = random.Random(42)
    cons = []
    for k in range(n_c):
        a = [(4, rnd.randrange(1, R))]
        b = [(3, rnd.randrange(1, R))] if k % 3 == 0 else [(0, 1)]
        c = [(2, rnd.randrange(1, R))] if k % 4 == 1 else []
        cons.append((a, b, c))
    cons[2][0].append((5, 9))
    cons[2][2].append((5, -BETA * 9 % R))               # w_5 = -beta u_5, v_5 = 0
    cons[6][0].extend([(6, 3), (8, R - 1), (6, 5)])     # wire 6 repeated inside A_6
    cons[7][1].extend([(7, 12345), (8, 2), (7, R - 12345)])  # wire 7 cancels inside B_7
    return cons, n_wires, 0, 0, 4


def _column_skew_system():
    """test_gpu_groth16_setup.py::test_column_skew"""
    n_c, n_wires = (1 << 10) - 1, 24
    rnd = random.Random(43)
    cons = []
    for k in range(n_c):
        other = 2 + k % (n_wires - 2)
        cons.append(([(1, rnd.randrange(1, R)), (other, 1)], [(1, R - 1), (0, rnd.randrange(R))], [(other, 2), (1, rnd.randrange(1, R))]))
    return cons, n_wires, 0, 0, 10


SYSTEMS = dict([("p%d" % p, functools.partial(_power_system, p)) for p in range(1, 9)] +
               [("column_edges", _column_edges_system), ("column_skew", _column_skew_system)])


@functools.lru_cache(maxsize=None)
def system(name):
    cons, n_wires, n_pub_out, n_pub_in, p = SYSTEMS[name]()
    r1 = PKG.R1cs(F.write_r1cs(n_wires, cons, n_pub_out=n_pub_out, n_pub_in=n_pub_in))
    assert r1.qap_info()["domain_power"] == p
    return cons, n_wires, n_pub_out + n_pub_in, p, r1


def assert_key(zkey, name, delta):
    """sections 1, 2, 3, 5 .. 9 against the Python Trapdoor at gamma = 1; sections 4 and 10 and the order against the trapdoor
    setup of the same values"""
    cons, n_wires, n_pub, p, r1 = system(name)
    T = GF.Trapdoor(cons, n_wires, n_pub, tau=TAU, alpha=ALPHA, beta=BETA, gamma=1, delta=delta)
    assert T.n == 1 << p
    ids, got = sections(zkey)
    assert ids == list(range(1, 11))
    _, want = sections(T.zkey)
    for sid in (1, 2, 3, 5, 6, 7, 8, 9):
        assert got[sid] == want[sid], "section %d differs" % sid
    _, trap = sections(PKG.groth16_setup(r1, (TAU, ALPHA, BETA, 1, delta)))
    assert got[4] == trap[4] and got[10] == trap[10] == NO_CONTRIBUTIONS
    return got


@pytest.mark.parametrize("delta", list(DELTAS))
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_keys(name, delta):
    _, _, _, p, r1 = system(name)
    assert_key(PKG.groth16_setup_ptau(r1, ptau(p + 1), DELTAS[delta], "compute"), name, DELTAS[delta])


@pytest.mark.parametrize("delta", list(DELTAS))
def test_key_from_a_larger_ceremony(delta):
    """p = 4 through a file of power p + 3: the prefixes are read, not the sections"""
    _, _, _, p, r1 = system("p4")
    assert_key(PKG.groth16_setup_ptau(r1, ptau(p + 3), DELTAS[delta]), "p4", DELTAS[delta])


def test_column_edges_points():
    """what test_gpu_groth16_setup.py::test_column_edges asserts about its wires, on the ptau key"""
    _, _, _, _, r1 = system("column_edges")
    _, sec = sections(PKG.groth16_setup_ptau(r1, ptau(5), DELTA_RANDOM))
    g1, g2 = lambda s, i: sec[s][64 * i:64 * i + 64], lambda i: sec[7][128 * i:128 * i + 128]  # noqa: E731
    assert not any(g1(5, 1)) and not any(g1(6, 1)) and not any(g2(1)) and not any(g1(8, 0))  # wire 1 nowhere
    assert not any(g1(5, 2)) and not any(g1(6, 2)) and any(g1(8, 1))   # wire 2: only C
    assert not any(g1(5, 3)) and any(g1(6, 3)) and any(g2(3))          # wire 3: only B
    assert any(g1(5, 5)) and not any(g1(8, 4))                         # wire 5: K = O
    assert any(g1(5, 6)) and not any(g1(6, 7)) and not any(g2(7))      # wire 6 adds up, wire 7 cancels


# -- the Lagrange source --------------------------------------------------------------------------------------------------------
def test_lagrange_file_and_compute_agree():
    _, _, _, p, r1 = system("p4")
    prepared = ptau(5, True)
    assert PKG.ptau_info(prepared)["prepared"] and not PKG.ptau_info(ptau(5))["prepared"]
    from_file = PKG.groth16_setup_ptau(r1, prepared, DELTA_RANDOM, "file")
    assert from_file == PKG.groth16_setup_ptau(r1, prepared, DELTA_RANDOM, "compute")
    assert from_file == PKG.groth16_setup_ptau(r1, prepared, DELTA_RANDOM, "auto")
    assert from_file == PKG.groth16_setup_ptau(r1, ptau(5), DELTA_RANDOM, "auto")
    assert_key(from_file, "p4", DELTA_RANDOM)
    # a larger prepared file: level p of sections 12 to 15 and level p + 1 of section 12, not their ends
    assert from_file == PKG.groth16_setup_ptau(r1, ptau(6, True), DELTA_RANDOM, "file")


def test_each_mode_reads_what_it_says():
    """sections 12 to 15 written from another tau: `compute` gives tau's key, `file` the A section of the other tau's"""
    cons, n_wires, n_pub, p, r1 = system("p4")
    mixed = ptau(5, True, TAU_OTHER)
    assert mixed != ptau(5, True)
    assert_key(PKG.groth16_setup_ptau(r1, mixed, DELTA_RANDOM, "compute"), "p4", DELTA_RANDOM)
    _, got = sections(PKG.groth16_setup_ptau(r1, mixed, DELTA_RANDOM, "file"))
    other = GF.Trapdoor(cons, n_wires, n_pub, tau=TAU_OTHER, alpha=ALPHA, beta=BETA, gamma=1, delta=DELTA_RANDOM)
    _, want = sections(other.zkey)
    assert got[5] == want[5] and got[6] == want[6] and got[7] == want[7] and got[8] == want[8] and got[9] == want[9]
    assert got[5] != sections(PKG.groth16_setup_ptau(r1, mixed, DELTA_RANDOM, "compute"))[1][5]
    assert sections(PKG.groth16_setup_ptau(r1, mixed, DELTA_RANDOM, "auto"))[1] == got


def test_mode_and_domain_refusals():
    _, _, _, _, r1 = system("p4")
    with pytest.raises(PKG.WitnessCalcError, match="no prepared sections"):
        PKG.groth16_setup_ptau(r1, ptau(5), 1, "file")
    for prepared in (False, True):
        with pytest.raises(PKG.WitnessCalcError, match=r"domain 2\^4 needs a ceremony of power 5 or more, this file has power 4"):
            PKG.groth16_setup_ptau(r1, ptau(4, prepared), 1)


@pytest.mark.parametrize("sid,unit,index,mode", ((2, 64, 31, "compute"), (2, 64, 9, "compute"), (3, 128, 15, "compute"), (4, 64, 15, "compute"),
                                                 (5, 64, 1, "compute"), (12, 64, 15, "file"), (12, 64, 30, "file"), (12, 64, 32, "file"),
                                                 (13, 128, 20, "file"), (14, 64, 22, "file"), (15, 64, 17, "file")))
def test_point_faults_found_on_the_device(sid, unit, index, mode):
    """p = 4: a point off its curve and, in each coordinate slot in turn, a coordinate >= q among the points read, named as the
    host check names them"""
    _, _, _, _, r1 = system("p4")
    secs = dict(ptau_sections(5, True))
    off = GF.lem(1) + GF.lem(3) if unit == 64 else GF.lem(1) + GF.lem(0) + GF.lem(1) + GF.lem(0)
    at_q = [bytes(32 * k) + Q.to_bytes(32, "little") + bytes(unit - 32 * k - 32) for k in range(unit // 32)]
    for fault, pattern in [(off, r"is not on the G%d curve" % (unit // 64))] + [(f, "has a coordinate >= q") for f in at_q]:
        body = secs[sid]
        bad = dict(secs)
        bad[sid] = body[:unit * index] + fault + body[unit * index + unit:]
        data = PF.assemble(bad)
        with pytest.raises(PKG.WitnessCalcError, match=r"section %d \([\w ]+\) point %d %s" % (sid, index, pattern)) as dev:
            PKG.groth16_setup_ptau(r1, data, 1, mode)
        with pytest.raises(PKG.WitnessCalcError) as host:
            PKG.ptau_check(data, 4, mode)
        assert str(dev.value) == str(host.value)
        other = "file" if mode == "compute" else "compute"
        assert PKG.groth16_setup_ptau(r1, data, 1, other) == PKG.groth16_setup_ptau(r1, ptau(5, True), 1, other)


# -- a drawn delta --------------------------------------------------------------------------------------------------------------
def _chain_system():
    """test_gpu_groth16_setup.py::_chain_system"""
    rnd = random.Random(46)
    shapes = [{"a": rnd.randrange(1, 4), "b": rnd.randrange(1, 4), "c": rnd.randrange(0, 3)} for _ in range(50)]
    pl = F.planted_system(rnd, 6, shapes, [1, R - 1, 2, F.MONT_R, None])
    return pl, F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=2)


def test_drawn_delta_through_the_pairing():
    pl, data = _chain_system()
    r1 = PKG.R1cs(data)
    assert r1.qap_info()["domain_power"] == 6
    z1, z2 = PKG.groth16_setup_ptau(r1, ptau(7)), PKG.groth16_setup_ptau(r1, ptau(7))
    (_, s1), (_, s2) = sections(z1), sections(z2)
    assert s1[2][DELTA1_AT:DELTA1_AT + 64] != s2[2][DELTA1_AT:DELTA1_AT + 64]
    assert s1[2][:DELTA1_AT] == s2[2][:DELTA1_AT] and s1[5] == s2[5] and s1[3] == s2[3] and s1[8] != s2[8] and s1[9] != s2[9]
    g = PKG.Groth16.setup_ptau(r1, ptau(7))
    assert g.info["n_public"] == 3 and g.info["n_vars"] == pl.n_wires
    vk = g.verifying_key()
    rnd = random.Random(47)
    rows = [pl.complete(rnd) for _ in range(8)]
    proofs = g.prove_batch(F.rows_array(rows))
    publics = [w[1:4] for w in rows]
    assert list(vk.verify_batch(proofs, publics)) == [PKG.VERIFY_VALID] * 8
    moved = [[p[0], (p[1] + 1) % R, p[2]] for p in publics]
    assert list(vk.verify_batch(proofs, moved)) == [PKG.VERIFY_EQUATION] * 8


def _wtns(w):
    img = b"wtns" + struct.pack("<II", 2, 2)
    img += struct.pack("<IQI", 1, 40, 32) + R.to_bytes(32, "little") + struct.pack("<I", len(w))
    return img + struct.pack("<IQ", 2, 32 * len(w)) + b"".join(x.to_bytes(32, "little") for x in w)


def test_cli_chain(tmp_path):
    """groth16-setup --ptau --delta, groth16-prove, groth16-verify on the files the first two wrote"""
    pl, data = _chain_system()
    (tmp_path / "c.r1cs").write_bytes(data)
    (tmp_path / "pot.ptau").write_bytes(ptau(7))
    (tmp_path / "d.txt").write_text("%d\n" % DELTA_RANDOM)
    (tmp_path / "t.txt").write_text("5 7 11 13 17\n")
    (tmp_path / "w.wtns").write_bytes(_wtns(pl.complete(random.Random(50))))
    path = lambda name: str(tmp_path / name)  # noqa: E731
    p = subprocess.run([os.path.join(BIN, "groth16-setup"), "--ptau", path("pot.ptau"), "--trapdoor", path("t.txt"), path("c.r1cs"), path("c.zkey")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "usage" in p.stderr and not (tmp_path / "c.zkey").exists()
    p = subprocess.run([os.path.join(BIN, "groth16-setup"), "--ptau", path("pot.ptau"), "--delta", path("d.txt"), path("c.r1cs"), path("c.zkey"),
                        path("vk.json")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p
    assert "forge" in p.stderr and "ceremony" in p.stderr
    zkey = (tmp_path / "c.zkey").read_bytes()
    assert zkey == PKG.groth16_setup_ptau(PKG.R1cs(data), ptau(7), DELTA_RANDOM)
    assert json.loads((tmp_path / "vk.json").read_text()) == PKG.Groth16VerifyingKey.from_zkey(zkey).to_json()
    subprocess.run([os.path.join(BIN, "groth16-prove"), path("c.r1cs"), path("c.zkey"), path("w.wtns"), path("proof.json"), path("public.json")],
                   check=True, timeout=300)
    p = subprocess.run([os.path.join(BIN, "groth16-verify"), path("vk.json"), path("public.json"), path("proof.json")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK!" in p.stdout, p


def test_phase_timer():
    _, _, _, _, r1 = system("p4")
    PKG.groth16_setup_ptau(r1, ptau(5, True), DELTA_RANDOM, "compute")
    ms = PKG.groth16_setup_ptau_phase_ms()
    assert list(ms) == list(PKG.GROTH16_SETUP_PTAU_PHASES) and len(ms) == 7
    assert all(math.isfinite(x) and x >= 0 for x in ms.values()), ms
    assert ms["idft_g1"] > 0 and ms["idft_g2"] > 0
    PKG.groth16_setup_ptau(r1, ptau(5, True), DELTA_RANDOM, "file")
    ms = PKG.groth16_setup_ptau_phase_ms()
    assert all(math.isfinite(x) and x >= 0 for x in ms.values()), ms
    assert ms["idft_g1"] == 0 and ms["idft_g2"] == 0 and ms["column_sums_g1"] > 0
