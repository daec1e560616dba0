"""The Groth16 key setup (r1cs/setup.hip, gwb_groth16_setup) on an MI355X against the existing Python: keys byte for byte
equal to tests/groth16_fixtures.py's Trapdoor at domain powers 1 to 8, section 4 against plain integers, hand-written column
edges (absent wires, one-matrix wires, a wire in every constraint, a C scalar of 0, nPub = 0, repeated wires), a skewed
column at 2^10, trapdoor edges, the fixed-base multiplication against Curve.gen_muls, and the whole chain setup -> prove ->
verify through the pairing with a drawn trapdoor, from Python and from the CLIs."""
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
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
R = F.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "circom-witnesscalc_amd")
NO_CONTRIBUTIONS = bytes(64) + struct.pack("<I", 0)

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


def trapdoor_of(seed):
    rnd = random.Random(seed)
    return tuple(rnd.randrange(1, R) for _ in range(5))


def reference(constraints, n_wires, n_pub, trap):
    tau, alpha, beta, gamma, delta = trap
    return GF.Trapdoor(constraints, n_wires, n_pub, tau=tau, alpha=alpha, beta=beta, gamma=gamma, delta=delta)


def assert_key_equal(zkey, T):
    """sections 1, 2, 3, 5 .. 9 byte for byte; section 10; the section order"""
    ids, got = sections(zkey)
    assert ids == list(range(1, 11))
    _, want = sections(T.zkey)
    for sid in (1, 2, 3, 5, 6, 7, 8, 9):
        assert got[sid] == want[sid], "section %d differs" % sid
    assert got[10] == NO_CONTRIBUTIONS


def setup_and_compare(constraints, n_wires, n_pub_out, n_pub_in, trap):
    r1 = PKG.R1cs(F.write_r1cs(n_wires, constraints, n_pub_out=n_pub_out, n_pub_in=n_pub_in))
    zkey = PKG.groth16_setup(r1, trap)
    T = reference(constraints, n_wires, n_pub_out + n_pub_in, trap)
    assert r1.qap_info()["domain_size"] == T.n
    assert_key_equal(zkey, T)
    return r1, zkey, T


@functools.lru_cache(maxsize=None)
def power_case(p):
    """the planted system of test_gpu_groth16.py::test_domain_powers for the domain 2^p, its key and its reference"""
    n_pub_in = 0 if p <= 2 else 2
    n_pub = n_pub_in + (0 if p <= 2 else 1)
    n_c = (1 << p) - n_pub - 1 - random.Random(p).randrange(0, 1 << (p - 1))
    rnd = random.Random(100 + p)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(n_c)]
    pl = F.planted_system(rnd, 6, shapes, [1, R - 1, 2, F.MONT_R, None])
    trap = trapdoor_of(200 + p)
    r1 = PKG.R1cs(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=n_pub - n_pub_in, n_pub_in=n_pub_in))
    return pl, n_pub, r1, PKG.groth16_setup(r1, trap), trap


@pytest.mark.parametrize("p", range(1, 9))
def test_domain_powers(p):
    pl, n_pub, r1, zkey, trap = power_case(p)
    T = reference(pl.constraints, pl.n_wires, n_pub, trap)
    assert T.n == 1 << p and r1.qap_info()["domain_size"] == T.n
    assert_key_equal(zkey, T)
    g = PKG.Groth16(zkey, r1)  # gwb_zkey_load accepts the file
    n_terms = sum(len(a) + len(b) for a, b, _ in pl.constraints)
    assert g.info == {"n_vars": pl.n_wires, "n_public": n_pub, "domain_size": 1 << p, "n_coefs": n_terms + n_pub + 1}


@pytest.mark.parametrize("p", (5, 8))
def test_section_4(p):
    """count, order and values of the coefficients: per constraint its A terms then its B terms as the file stores them, then
    the public rows; value R^2 mod r, little-endian"""
    pl, n_pub, _, zkey, _ = power_case(p)
    want = []
    for k, (a, b, _) in enumerate(pl.constraints):
        want += [(0, k, wire, c % R) for wire, c in F.terms(a)]
        want += [(1, k, wire, c % R) for wire, c in F.terms(b)]
    want += [(0, len(pl.constraints) + s, s, 1) for s in range(n_pub + 1)]
    body = sections(zkey)[1][4]
    count = struct.unpack_from("<I", body, 0)[0]
    assert count == len(want) and len(body) == 4 + 44 * count
    rr_inv = pow(F.MONT_R2, -1, R)
    seen = set()
    for i, (m, k, s, v) in enumerate(want):
        gm, gk, gs = struct.unpack_from("<III", body, 4 + 44 * i)
        stored = int.from_bytes(body[16 + 44 * i:48 + 44 * i], "little")
        assert (gm, gk, gs) == (m, k, s), i
        assert stored < R and stored * rr_inv % R == v, i
        seen.add(v)
    assert {1, R - 1, F.MONT_R} <= seen and len(seen) > 8  # the pool's edge coefficients and random ones all occurred


def test_column_edges():
    """p = 4, nPub = 0: wire 1 nowhere (A, B1, B2 and C at infinity), wire 2 only in C, wire 3 only in B, wire 4 in A of every
    constraint, wire 5 with beta u + alpha v + w = 0 (C at infinity), wire 6 twice in one combination, wire 7 a cancelling pair"""
    trap = trapdoor_of(41)
    beta = trap[2]
    n_c, n_wires = 10, 9
    rnd = random.Random(42)
    cons = []
    for k in range(n_c):
        a = [(4, rnd.randrange(1, R))]
        b = [(3, rnd.randrange(1, R))] if k % 3 == 0 else [(0, 1)]
        c = [(2, rnd.randrange(1, R))] if k % 4 == 1 else []
        cons.append((a, b, c))
    cons[2][0].append((5, 9))
    cons[2][2].append((5, -beta * 9 % R))               # w_5 = -beta u_5, v_5 = 0
    cons[6][0].extend([(6, 3), (8, R - 1), (6, 5)])     # wire 6 repeated inside A_6
    cons[7][1].extend([(7, 12345), (8, 2), (7, R - 12345)])  # wire 7 cancels inside B_7
    r1, zkey, T = setup_and_compare(cons, n_wires, 0, 0, trap)
    assert T.n == 16 and r1.info["n_pub_out"] + r1.info["n_pub_in"] == 0
    _, sec = sections(zkey)
    g1, g2 = lambda s, i: sec[s][64 * i:64 * i + 64], lambda i: sec[7][128 * i:128 * i + 128]  # noqa: E731
    assert not any(g1(5, 1)) and not any(g1(6, 1)) and not any(g2(1)) and not any(g1(8, 0))  # wire 1; C_0 is wire 1's
    assert not any(g1(5, 2)) and not any(g1(6, 2)) and any(g1(8, 1))   # wire 2: only w
    assert not any(g1(5, 3)) and any(g1(6, 3)) and any(g2(3))          # wire 3: only v
    assert any(g1(5, 5)) and not any(g1(8, 4))                         # wire 5: u != 0, C scalar 0
    assert any(g1(5, 6)) and not any(g1(6, 7)) and not any(g2(7))      # wire 6 adds up, wire 7 cancels
    assert len(sec[3]) == 64 and any(sec[3])                           # IC_0 alone


def test_column_skew():
    """p = 10: wire 1 has a term in A, B and C of all 2^10 - 1 constraints, every other wire a few"""
    n_c, n_wires = (1 << 10) - 1, 24
    rnd = random.Random(43)
    cons = []
    for k in range(n_c):
        other = 2 + k % (n_wires - 2)
        cons.append(([(1, rnd.randrange(1, R)), (other, 1)], [(1, R - 1), (0, rnd.randrange(R))], [(other, 2), (1, rnd.randrange(1, R))]))
    r1, _, T = setup_and_compare(cons, n_wires, 0, 0, trapdoor_of(44))
    assert T.n == 1 << 10


@pytest.mark.parametrize("trap", [(2, 1, R - 1, 1, 1), (2, 1, R - 1, 1, R - 1)], ids=["delta_1", "delta_r_minus_1"])
def test_trapdoor_edges(trap):
    pl, n_pub, r1, _, _ = power_case(4)
    assert_key_equal(PKG.groth16_setup(r1, trap), reference(pl.constraints, pl.n_wires, n_pub, trap))


# -- the fixed-base multiplication --------------------------------------------------------------------------------------------
def _gen_mul_scalars():
    """4 097 scalars below 2^256: the edges with zeros between them first, then seeded values of one to three nonzero bytes"""
    rnd = random.Random(45)
    full = (1 << 256) - 1
    edge = [R - 1, 0, 1, 2, R, R + 1, full, 0, full % R, int.from_bytes(b"\x01" * 32, "little")]
    for w in range(32):
        edge += [1 << (8 * w), (1 << (8 * w)) - 1]
    edge += [rnd.randrange(R) for _ in range(64)]
    ks = []
    for i, k in enumerate(edge):
        ks.append(k)
        if i % 5 == 4:
            ks.append(0)  # zeros next to nonzero values: a shared inversion sees both
    while len(ks) < 4097:
        k = 0
        for _ in range(rnd.randrange(1, 4)):
            k |= rnd.randrange(1, 256) << (8 * rnd.randrange(32))
        ks.append(k if len(ks) % 7 else 0)
    assert len(ks) == 4097 and ks[0] == R - 1 and 0 in ks[:65] and ks[64] != 0
    return ks


def _point_bytes(p, words):
    if p is None:
        return bytes(32 * words)
    cs = p if words == 2 else (p[0][0], p[0][1], p[1][0], p[1][1])
    return b"".join(x.to_bytes(32, "little") for x in cs)


@functools.lru_cache(maxsize=None)
def _gen_mul_reference(group):
    curve, words = (GF.G1, 2) if group == 1 else (GF.G2, 4)
    pts = curve.gen_muls(_gen_mul_scalars())
    assert pts[1] is None and pts[4] is None and pts[0] is not None  # 0 and r give infinity
    return np.frombuffer(b"".join(_point_bytes(p, words) for p in pts), dtype=np.uint8).reshape(len(pts), 32 * words)


@pytest.mark.parametrize("group", (1, 2))
def test_gen_mul_batch_device(group):
    """1 scalar (a partial wave), 65 (more than a wave), 4 097 (more than a block)"""
    import torch
    ks = _gen_mul_scalars()
    want = _gen_mul_reference(group)
    arr = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ks), dtype=np.uint8).reshape(len(ks), 32)
    for n in (1, 65, 4097):
        d = torch.from_numpy(arr[:n].copy()).cuda()
        got = PKG.bn254_gen_mul_batch_device(d, group)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.shape == (n, 64 * group)
        assert np.array_equal(got, want[:n]), "group %d, %d scalars: rows %s differ" % (
            group, n, np.nonzero((got != want[:n]).any(axis=1))[0][:8])
    assert PKG.bn254_gen_mul_batch_device(torch.empty((0, 32), dtype=torch.uint8, device="cuda"), group).shape == (0, 64 * group)
    with pytest.raises(PKG.WitnessCalcError, match="group"):
        PKG.bn254_gen_mul_batch_device(d, 3)


# -- through the pairing ------------------------------------------------------------------------------------------------------
def _chain_system():
    rnd = random.Random(46)
    shapes = [{"a": rnd.randrange(1, 4), "b": rnd.randrange(1, 4), "c": rnd.randrange(0, 3)} for _ in range(50)]
    pl = F.planted_system(rnd, 6, shapes, [1, R - 1, 2, F.MONT_R, None])
    return pl, F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=2)


def test_drawn_trapdoor_through_the_pairing():
    pl, data = _chain_system()
    r1 = PKG.R1cs(data)
    assert r1.qap_info()["domain_power"] == 6
    g = PKG.Groth16.setup(r1)
    assert g.info["n_public"] == 3 and g.info["n_vars"] == pl.n_wires
    vk = g.verifying_key()
    rnd = random.Random(47)
    rows = [pl.complete(rnd) for _ in range(8)]
    proofs = g.prove_batch(F.rows_array(rows))
    publics = [w[1:4] for w in rows]
    assert list(vk.verify_batch(proofs, publics)) == [PKG.VERIFY_VALID] * 8
    moved = [[p[0], (p[1] + 1) % R, p[2]] for p in publics]
    assert list(vk.verify_batch(proofs, moved)) == [PKG.VERIFY_EQUATION] * 8
    # a row that violates a constraint: its proof follows the formula and fails the equation
    bad = None
    for f in pl.free:
        cand = list(rows[0])
        cand[f] = (cand[f] + 1) % R
        if r1.check_batch(F.rows_array([cand]))[0][0] != PKG.R1CS_SATISFIED:
            bad = cand
            break
    assert bad is not None
    assert list(vk.verify_batch(g.prove_batch(F.rows_array([bad])), [bad[1:4]])) == [PKG.VERIFY_EQUATION]
    # drawn keys differ; an explicit trapdoor is reproducible
    z1, z2 = PKG.groth16_setup(r1), PKG.groth16_setup(r1)
    assert sections(z1)[1][2] != sections(z2)[1][2]
    trap = trapdoor_of(48)
    assert PKG.groth16_setup(r1, trap) == PKG.groth16_setup(r1, trap)


def _wtns(w):
    img = b"wtns" + struct.pack("<II", 2, 2)
    img += struct.pack("<IQI", 1, 40, 32) + R.to_bytes(32, "little") + struct.pack("<I", len(w))
    return img + struct.pack("<IQ", 2, 32 * len(w)) + b"".join(x.to_bytes(32, "little") for x in w)


def test_cli_chain(tmp_path):
    """groth16-setup --trapdoor, groth16-prove, groth16-verify on the files the first two wrote"""
    pl, data = _chain_system()
    trap = trapdoor_of(49)
    (tmp_path / "c.r1cs").write_bytes(data)
    (tmp_path / "t.txt").write_text(" ".join(str(x) for x in trap) + "\n")
    (tmp_path / "w.wtns").write_bytes(_wtns(pl.complete(random.Random(50))))
    path = lambda name: str(tmp_path / name)  # noqa: E731
    p = subprocess.run([os.path.join(BIN, "groth16-setup"), "--trapdoor", path("t.txt"), path("c.r1cs"), path("c.zkey"), path("vk.json")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p
    assert "forge" in p.stderr
    zkey = (tmp_path / "c.zkey").read_bytes()
    assert zkey == PKG.groth16_setup(PKG.R1cs(data), trap)
    assert json.loads((tmp_path / "vk.json").read_text()) == PKG.Groth16VerifyingKey.from_zkey(zkey).to_json()
    subprocess.run([os.path.join(BIN, "groth16-prove"), path("c.r1cs"), path("c.zkey"), path("w.wtns"), path("proof.json"), path("public.json")],
                   check=True, timeout=300)
    p = subprocess.run([os.path.join(BIN, "groth16-verify"), path("vk.json"), path("public.json"), path("proof.json")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK!" in p.stdout, p


def test_phase_timer():
    _, _, r1, _, trap = power_case(5)
    PKG.groth16_setup(r1, trap)
    ms = PKG.groth16_setup_phase_ms()
    assert list(ms) == list(PKG.GROTH16_SETUP_PHASES) and len(ms) == 5
    assert all(math.isfinite(x) and x >= 0 for x in ms.values()), ms
