"""The Groth16 verifier's host side without a GPU: the plain-Python pairing oracle (tests/bn254_pairing.py: non-degenerate, of
order r, bilinear, the flat <-> tower map a ring isomorphism), the tower constant generator against the committed .inc, the
verifying-key loader's refusals (coordinate >= q, off-curve points, a twist point outside the subgroup, the IC count, a mutant
fuzz), the Python JSON readers, and the groth16-verify CLI's exit-2 cases."""
import json
import os
import random
import subprocess
import sys

import pytest

import cwc_import
from tests import bn254_pairing as BP
from tests import groth16_fixtures as GF

PKG = cwc_import.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "circom-witnesscalc_amd", "groth16-verify")
R, Q = GF.R, GF.Q


# -- the oracle -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e11():
    return BP.pairing(GF.G1_GEN, GF.G2_GEN)


def test_pairing_non_degenerate_of_order_r(e11):
    assert e11 != BP.ONE
    assert BP.power(e11, R) == BP.ONE


@pytest.mark.parametrize("a,b", [(2, 3), (R - 1, 5), (123456789, 987654321)])
def test_pairing_bilinear(e11, a, b):
    pa = GF.G1.to_affine(GF.G1.mul(GF.G1_GEN, a))
    qb = GF.G2.to_affine(GF.G2.mul(GF.G2_GEN, b))
    assert BP.pairing(pa, qb) == BP.power(e11, a * b)


def test_pairing_of_a_negated_point(e11):
    assert BP.pairing(GF.G1.neg_aff(GF.G1_GEN), GF.G2_GEN) == BP.inv(e11)
    assert BP.mul(BP.pairing(GF.G1.neg_aff(GF.G1_GEN), GF.G2_GEN), e11) == BP.ONE


def test_flat_tower_map_is_a_ring_isomorphism():
    rnd = random.Random(3)
    for _ in range(5):
        x = tuple(rnd.randrange(Q) for _ in range(12))
        y = tuple(rnd.randrange(Q) for _ in range(12))
        tx, ty = BP.to_tower(x), BP.to_tower(y)
        assert BP.from_tower(tx) == x
        assert BP.from_tower([(s + t) % Q for s, t in zip(tx, ty)]) == BP.add(x, y)
        assert BP.from_tower(BP.tower_mul(tx, ty)) == BP.mul(x, y)
        assert BP.gt_from_bytes(BP.gt_bytes(x)) == x
    assert BP.to_tower(BP.ONE) == [1] + [0] * 11


def test_twist_point_outside_the_subgroup():
    p = BP.twist_point_outside_subgroup(random.Random(4))
    assert GF.G2.on_curve(p) and not GF.G2.is_inf(GF.G2.mul(p, R))


def test_generator_reproduces_the_committed_inc(tmp_path):
    out = tmp_path / "c.inc"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "codegen", "gen_fq12_consts.py"), str(out)],
                          stdout=subprocess.DEVNULL)
    committed = os.path.join(ROOT, "circom-witnesscalc_amd", "r1cs", "fq12_consts_gfx950.inc")
    assert out.read_bytes() == open(committed, "rb").read()


# -- the key loader ---------------------------------------------------------------------------------------------------------------
def _i(x):
    return x.to_bytes(32, "little")


def _g1b(p):
    return bytes(64) if p is None else _i(p[0]) + _i(p[1])


def _g2b(p):
    return bytes(128) if p is None else b"".join(_i(x) for x in (p[0][0], p[0][1], p[1][0], p[1][1]))


def _key_points(n_public, seed=1):
    rnd = random.Random(seed)
    g1 = GF.G1.gen_muls([rnd.randrange(1, R) for _ in range(n_public + 2)])
    g2 = GF.G2.gen_muls([rnd.randrange(1, R) for _ in range(3)])
    return _g1b(g1[0]) + b"".join(map(_g2b, g2)) + b"".join(map(_g1b, g1[1:]))


def test_key_loads_and_round_trips():
    pts = _key_points(3)
    vk = PKG.Groth16VerifyingKey(pts, 3)
    assert vk.n_public == 3 and vk.points() == pts
    assert PKG.Groth16VerifyingKey(_key_points(0), 0).n_public == 0


def _refused(pts, n, match):
    with pytest.raises(PKG.WitnessCalcError, match=match):
        PKG.Groth16VerifyingKey(pts, n)


def test_key_refusals():
    pts = bytearray(_key_points(2))
    bad = bytearray(pts)
    bad[0:32] = _i(int.from_bytes(pts[0:32], "little") + Q)
    _refused(bad, 2, "alpha1 has a coordinate >= q")
    bad = bytearray(pts)
    bad[64 + 96:64 + 128] = _i((int.from_bytes(pts[64 + 96:64 + 128], "little") + 1) % Q)
    _refused(bad, 2, "beta2 is not on the G2 twist curve")
    bad = bytearray(pts)
    bad[448 + 64 + 32:448 + 128] = _i((int.from_bytes(pts[448 + 96:448 + 128], "little") + 1) % Q)
    _refused(bad, 2, r"IC\[1\] is not on the G1 curve")
    bad = bytearray(pts)
    bad[320:448] = _g2b(BP.twist_point_outside_subgroup(random.Random(6)))
    _refused(bad, 2, "delta2 is not in the order-r subgroup")
    _refused(pts, 3, "3 IC points for nPublic 3")
    _refused(pts[:-64], 2, "2 IC points for nPublic 2")
    _refused(pts[:-1], 2, "bytes for nPublic 2")


def test_key_mutant_fuzz():
    """single-byte mutants of a valid key: each loads or is refused with a verifying-key message, never anything else"""
    pts = _key_points(1, seed=8)
    rnd = random.Random(9)
    refused = 0
    for _ in range(60):
        m = bytearray(pts)
        m[rnd.randrange(len(m))] ^= 1 << rnd.randrange(8)
        try:
            PKG.Groth16VerifyingKey(bytes(m), 1)
        except PKG.WitnessCalcError as e:
            assert str(e).startswith("verifying key: "), str(e)
            refused += 1
    assert refused >= 55  # a flipped coordinate bit leaves the curve (or q) except by chance


def test_key_from_zkey_and_json_on_the_host():
    """from_zkey converts the zkey's Montgomery points; from_json reads snarkjs's shape (vk_alphabeta_12 ignored)"""
    rnd = random.Random(11)
    g1 = GF.G1.gen_muls([rnd.randrange(1, R) for _ in range(4)])
    g2 = GF.G2.gen_muls([rnd.randrange(1, R) for _ in range(3)])
    zk = GF.write_zkey(4, 1, 2, g1[0], g1[1], g2[0], g2[1], g1[2], g2[2], [g1[3], None], [None] * 4, [None] * 4, [None] * 4,
                       [None] * 2, [None] * 2)
    vk = PKG.Groth16VerifyingKey.from_zkey(zk)
    assert vk.points() == _g1b(g1[0]) + _g2b(g2[0]) + _g2b(g2[1]) + _g2b(g2[2]) + _g1b(g1[3]) + bytes(64)
    j = {"protocol": "groth16", "curve": "bn128", "nPublic": 1, "vk_alphabeta_12": "ignored",
         "vk_alpha_1": [str(g1[0][0]), str(g1[0][1]), "1"],
         "vk_beta_2": [[str(g2[0][0][0]), str(g2[0][0][1])], [str(g2[0][1][0]), str(g2[0][1][1])], ["1", "0"]],
         "vk_gamma_2": [[str(g2[1][0][0]), str(g2[1][0][1])], [str(g2[1][1][0]), str(g2[1][1][1])], ["1", "0"]],
         "vk_delta_2": [[str(g2[2][0][0]), str(g2[2][0][1])], [str(g2[2][1][0]), str(g2[2][1][1])], ["1", "0"]],
         "IC": [[str(g1[3][0]), str(g1[3][1]), "1"], ["0", "1", "0"]]}
    assert PKG.Groth16VerifyingKey.from_json(j).points() == vk.points()
    with pytest.raises(PKG.WitnessCalcError, match="z must be"):
        PKG.Groth16VerifyingKey.from_json(dict(j, vk_alpha_1=[j["vk_alpha_1"][0], j["vk_alpha_1"][1], "2"]))
    with pytest.raises(PKG.WitnessCalcError, match="IC points"):
        PKG.Groth16VerifyingKey.from_json(dict(j, nPublic=2))


# -- the CLI ---------------------------------------------------------------------------------------------------------------------
def _run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_cli_exit_2(tmp_path):
    assert _run().returncode == 2
    assert _run("a", "b").returncode == 2
    assert _run("a", "b", "c", "d").returncode == 2
    p = _run(tmp_path / "none.json", tmp_path / "p.json", tmp_path / "q.json")
    assert p.returncode == 2 and "cannot read" in p.stderr
    vk = tmp_path / "vk.json"
    pub = tmp_path / "public.json"
    proof = tmp_path / "proof.json"
    pts = _key_points(1)
    key = PKG.Groth16VerifyingKey(pts, 1)
    j = {"protocol": "groth16", "curve": "bn128", "nPublic": 1, "vk_alpha_1": PKG._json_g1(pts[:64]),
         "vk_beta_2": PKG._json_g2(pts[64:192]), "vk_gamma_2": PKG._json_g2(pts[192:320]),
         "vk_delta_2": PKG._json_g2(pts[320:448]), "IC": [PKG._json_g1(pts[448:512]), PKG._json_g1(pts[512:576])]}
    assert key.n_public == 1
    good_proof = PKG.proof_json(bytes(256))
    cases = [
        ("{not json", ["1"], good_proof, "JSON"),
        (j, "[1, ", good_proof, "JSON"),
        (j, ["1"], "{\"pi_a\": [1, 2, 3]", "JSON"),
        (dict(j, protocol="plonk"), ["1"], good_proof, "protocol"),
        (dict(j, nPublic=2), ["1", "2"], good_proof, "IC points"),
        (j, ["1", "2"], good_proof, "public signals"),
        (j, ["x"], good_proof, "not a decimal integer"),
        (j, [str(1 << 256)], good_proof, "above 2"),
        (j, ["1"], {"pi_a": good_proof["pi_a"], "pi_b": good_proof["pi_b"]}, "pi_c"),
        (j, ["1"], dict(good_proof, pi_a=["1", "2", "5"]), "z must be"),
        (dict(j, vk_alpha_1=[str(Q), "1", "1"]), ["1"], good_proof, "coordinate >= q"),
    ]
    for k, p_, pr, msg in cases:
        vk.write_text(k if isinstance(k, str) else json.dumps(k))
        pub.write_text(p_ if isinstance(p_, str) else json.dumps(p_))
        proof.write_text(pr if isinstance(pr, str) else json.dumps(pr))
        res = _run(vk, pub, proof)
        assert res.returncode == 2 and msg in res.stderr, (msg, res.returncode, res.stderr)


def test_every_verifier_kernel_without_scratch(tmp_path):
    """hipcc -Rpass-analysis=kernel-resource-usage on r1cs/verify.hip: each of its seven kernels reports ScratchSize 0"""
    import re
    src = os.path.join(ROOT, "circom-witnesscalc_amd", "r1cs", "verify.hip")
    p = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "v.o")],
                       capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stderr)]
    kernels = {n for n in names if "kernel" in n}
    assert len(kernels) == 7 and len(scratch) == len(names), (names, scratch)
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
