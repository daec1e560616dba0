"""Compressed Groth16 proofs and verifying keys on an MI355X (r1cs/codec.hip, include/graph_witness_groth16_compressed.h), on the
tiny trapdoor key of tests/groth16_fixtures.py: prove_batch_compressed against the model's compression of prove_batch with the
same r, s; verify_batch_compressed against verify_batch on the raw proofs; every status and the rule order PUBLIC, POINT,
SUBGROUP, EQUATION on tampered encodings; the compressed key there and back, its refusals; and the three CLIs in a chain.
Expected bytes come from tests/point_codec_cases.py alone."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import cwc_import
from tests import bn254_pairing as BP
from tests import groth16_fixtures as GF
from tests import point_codec_cases as PC
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
pytestmark = pytest.mark.gpu
R, Q = GF.R, GF.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "circom-witnesscalc_amd")
VALID, PUBLIC, POINT, SUBGROUP, EQUATION = (PKG.VERIFY_VALID, PKG.VERIFY_PUBLIC, PKG.VERIFY_POINT, PKG.VERIFY_SUBGROUP,
                                            PKG.VERIFY_EQUATION)
N_PUB = 3


@pytest.fixture(scope="module")
def system():
    """a planted system of 12 constraints with its trapdoor key, 65 witness rows (the last one unsatisfied) and their r, s, the raw
    proofs and their statuses: the reference, computed once"""
    rnd = random.Random(80)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(12)]
    pl = F.planted_system(rnd, 6, shapes, [1, R - 1, 2, F.MONT_R, None])
    r1 = PKG.R1cs(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=2))
    T = GF.Trapdoor(pl.constraints, pl.n_wires, N_PUB, seed=80)
    g = PKG.Groth16(T.zkey, r1)
    rows = [pl.complete(rnd) for _ in range(65)]
    bad = list(rows[64])
    bad[pl.free[0]] = (bad[pl.free[0]] + 1) % R
    rows[64] = bad
    rs = [(rnd.randrange(R), rnd.randrange(R)) for _ in rows]
    vk = g.verifying_key()
    pubs = [w[1:1 + N_PUB] for w in rows]
    raw = g.prove_batch(F.rows_array(rows), rs=rs)
    status = vk.verify_batch(raw, pubs)
    assert list(status) == [VALID] * 64 + [EQUATION]
    return dict(pl=pl, T=T, g=g, vk=vk, rows=rows, rs=rs, pubs=pubs, raw=raw, status=status)


def _model(raw):
    return np.frombuffer(b"".join(PC.proof_compress(r.tobytes()) for r in raw), dtype=np.uint8).reshape(len(raw), 128).copy()


def _verify_both(vk, cproofs, pubs):
    """the host and the device entry points of the compressed verifier, which must agree"""
    import torch
    host = vk.verify_batch_compressed(cproofs, pubs)
    pa = PKG._public_array(pubs, len(pubs), vk.n_public)
    dev = vk.verify_batch_compressed_device(torch.from_numpy(np.ascontiguousarray(cproofs)).cuda(), torch.from_numpy(pa).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(host, dev.cpu().numpy().astype(np.uint32))
    return list(host)


# -- batches -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", (1, 64, 65))
def test_prove_and_verify_compressed(system, batch):
    s = system
    rows, rs, pubs = s["rows"][-batch:], s["rs"][-batch:], s["pubs"][-batch:]   # (the unsatisfied row is in every batch)
    got = s["g"].prove_batch_compressed(F.rows_array(rows), rs=rs)
    assert got.shape == (batch, 128) and got.dtype == np.uint8
    assert np.array_equal(got, _model(s["raw"][-batch:]))
    assert _verify_both(s["vk"], got, pubs) == list(s["status"][-batch:])
    assert np.array_equal(PKG.groth16_compress_proofs(s["raw"][-batch:]), got)
    back, dec = PKG.groth16_decompress_proofs(got)
    assert np.array_equal(back, s["raw"][-batch:]) and not dec.any()


def test_batch_zero(system):
    import torch
    vk = system["vk"]
    assert vk.verify_batch_compressed(np.zeros((0, 128), np.uint8), []).shape == (0,)
    d = vk.verify_batch_compressed_device(torch.zeros((0, 128), dtype=torch.uint8, device="cuda"),
                                          torch.zeros((0, N_PUB, 32), dtype=torch.uint8, device="cuda"))
    assert tuple(d.shape) == (0,)
    with pytest.raises(PKG.WitnessCalcError, match="4 public signals in row 0"):
        vk.verify_batch_compressed(np.zeros((1, 128), np.uint8), [[1, 2, 3, 4]])


# -- statuses ------------------------------------------------------------------------------------------------------------------------
def test_statuses_and_their_order(system):
    s = system
    n = 10
    c = _model(s["raw"][:n])
    pubs = [list(p) for p in s["pubs"][:n]]
    want = [VALID] * n
    rnd = random.Random(81)
    # 1: the sign bit of A flipped: -A, on the curve, decodes -> EQUATION
    c[1, 31] ^= 0x80
    want[1] = EQUATION
    # 2: A's x replaced by an x without a root -> POINT
    c[2, :32] = np.frombuffer(PC.no_root_x(1, rnd).to_bytes(32, "little"), np.uint8)
    want[2] = POINT
    # 3: both flags on C -> POINT
    c[3, 127] |= 0xc0
    want[3] = POINT
    # 4: B a twist point outside the order-r subgroup, compressed by the model -> SUBGROUP
    out = BP.twist_point_outside_subgroup(random.Random(5))
    c[4, 32:96] = np.frombuffer(PC.g2_compress(out), np.uint8)
    want[4] = SUBGROUP
    # 5: a public signal >= r and a refused point -> PUBLIC, the first rule
    pubs[5][1] += R
    c[5, 127] |= 0xc0
    want[5] = PUBLIC
    # 6: a refused A beside a B outside the subgroup -> POINT comes before SUBGROUP
    c[6, 31] |= 0xc0
    c[6, 32:96] = np.frombuffer(PC.g2_compress(out), np.uint8)
    want[6] = POINT
    # 7: every point at infinity decodes, and gets what the raw path gives the all-zero proof
    c[7] = np.frombuffer(PC.g1_compress(None) + PC.g2_compress(None) + PC.g1_compress(None), np.uint8)
    want[7] = int(s["vk"].verify_batch(np.zeros((1, 256), np.uint8), [pubs[7]])[0])
    assert want[7] == EQUATION
    # 8: the infinity flag on B with a bit of x left -> POINT
    c[8, 95] |= 0x40
    want[8] = POINT
    # 9: a public signal >= r alone -> PUBLIC
    pubs[9][0] = R
    want[9] = PUBLIC
    assert _verify_both(s["vk"], c, pubs) == want
    back, dec = PKG.groth16_decompress_proofs(c)
    assert [int(x) for x in dec] == [POINT if i in (2, 3, 5, 6, 8) else VALID for i in range(n)]
    assert back[4, 64:192].tobytes() == PC.g2_bytes(out) and not back[7].any() and not back[2, :64].any() and back[2, 64:].tobytes() == s["raw"][2, 64:].tobytes()


# -- keys ----------------------------------------------------------------------------------------------------------------------------
def test_compressed_key_there_and_back(system):
    vk = system["vk"]
    c = vk.to_compressed()
    assert len(c) == 232 + 32 * (N_PUB + 1) and c == PC.key_compress(vk.points(), N_PUB)
    again = PKG.Groth16VerifyingKey.from_compressed(c)
    assert again.n_public == N_PUB and again.points() == vk.points()
    got = again.verify_batch_compressed(_model(system["raw"][-3:]), system["pubs"][-3:])
    assert list(got) == list(system["status"][-3:])


def test_compressed_key_refusals(system):
    c = system["vk"].to_compressed()

    def refused(data, match):
        with pytest.raises(PKG.WitnessCalcError, match=match) as e:
            PKG.Groth16VerifyingKey.from_compressed(bytes(data))
        assert str(e.value).startswith("verifying key:")

    refused(c[:-1], "359 bytes")
    refused(c[:200], "200 bytes")
    refused(b"", "0 bytes")
    refused(c[:-32], "length prefix counts 4 IC points, the bytes hold 3")
    refused(c + c[-32:], "length prefix counts 4 IC points, the bytes hold 5")
    for name, lo, width in (("alpha1", 0, 32), ("beta2", 32, 64), ("gamma2", 96, 64), ("delta2", 160, 64), (r"IC\[3\]", 232 + 96, 32)):
        bad = bytearray(c)
        bad[lo + width - 1] |= 0xc0
        refused(bad, name + " is not a valid compressed point")
    bad = bytearray(c)
    bad[232:264] = PC.no_root_x(1, random.Random(82)).to_bytes(32, "little")
    refused(bad, r"IC\[0\] is not a valid compressed point")
    bad = bytearray(c)   # what gwb_g16vk_load refuses comes through: a G2 key point outside the subgroup
    bad[96:160] = PC.g2_compress(BP.twist_point_outside_subgroup(random.Random(5)))
    refused(bad, "gamma2 is not in the order-r subgroup")


# -- the CLIs ------------------------------------------------------------------------------------------------------------------------
def _run(tool, *args):
    return subprocess.run(["timeout", "-k", "10", "300", os.path.join(BIN, tool)] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_chain(system, tmp_path):
    s = system
    pl, w = s["pl"], s["rows"][0]
    img = b"wtns" + (2).to_bytes(4, "little") + (2).to_bytes(4, "little")
    img += (1).to_bytes(4, "little") + (40).to_bytes(8, "little") + (32).to_bytes(4, "little") + R.to_bytes(32, "little")
    img += pl.n_wires.to_bytes(4, "little")
    img += (2).to_bytes(4, "little") + (32 * pl.n_wires).to_bytes(8, "little") + b"".join(x.to_bytes(32, "little") for x in w)
    (tmp_path / "c.zkey").write_bytes(s["T"].zkey)
    (tmp_path / "c.r1cs").write_bytes(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=2))
    (tmp_path / "w.wtns").write_bytes(img)
    vkb, proof, pub = tmp_path / "vk.bin", tmp_path / "proof.bin", tmp_path / "public.json"
    p = _run("groth16-setup", "--export-vk", "--compressed", tmp_path / "c.zkey", vkb)
    assert p.returncode == 0, p.stderr
    assert vkb.read_bytes() == s["vk"].to_compressed()
    p = _run("groth16-prove", "--compressed", tmp_path / "c.r1cs", tmp_path / "c.zkey", tmp_path / "w.wtns", proof, pub)
    assert p.returncode == 0, p.stderr
    assert len(proof.read_bytes()) == 128 and json.loads(pub.read_text()) == [str(x) for x in w[1:1 + N_PUB]]
    p = _run("groth16-verify", "--compressed", vkb, pub, proof)
    assert p.returncode == 0 and p.stdout.strip() == "OK!", p.stdout + p.stderr
    flipped = bytearray(proof.read_bytes())
    flipped[31] ^= 0x80
    (tmp_path / "flipped.bin").write_bytes(flipped)
    p = _run("groth16-verify", "--compressed", vkb, pub, tmp_path / "flipped.bin")
    assert p.returncode == 1 and "EQUATION" in p.stdout, p.stdout + p.stderr
    (tmp_path / "short.bin").write_bytes(proof.read_bytes()[:127])
    p = _run("groth16-verify", "--compressed", vkb, pub, tmp_path / "short.bin")
    assert p.returncode == 2 and "127 bytes" in p.stderr, p.stdout + p.stderr
    p = _run("groth16-verify", vkb, pub, proof, "--compressed")   # the flag comes first
    assert p.returncode == 2 and "usage" in p.stderr
