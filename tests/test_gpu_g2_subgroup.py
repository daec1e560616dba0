"""G2 subgroup membership on an MI355X (r1cs/subgroup.hip): the aid gwb_bn254_g2_check_batch_device in both forms and both
methods against Python's [r] P = O on every point class of tests/g2_subgroup_fixtures.py, at sizes that cross a block of 64;
Groth16.check_g2 on small keys with planted points; ptau_check_g2 on power-3 and power-7 files with one G2 point swapped, in
every Lagrange mode, across the pieces of the upload; and the CLIs' --check-g2.  Expected statuses come from Python alone."""
import functools
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import cwc_import
from tests import bn254_pairing as BP
from tests import g2_subgroup_fixtures as SF
from tests import groth16_fixtures as GF
from tests import ptau_fixtures as PF
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
Q, R = GF.Q, GF.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "circom-witnesscalc_amd")
VALID, POINT, SUBGROUP = PKG.VERIFY_VALID, PKG.VERIFY_POINT, PKG.VERIFY_SUBGROUP
_rnd = random.Random(400)
TAU, ALPHA, BETA, DELTA = (_rnd.randrange(2, R) for _ in range(4))
SUB = "is not in the order-r subgroup of G2"

pytestmark = pytest.mark.gpu


# -- inputs ------------------------------------------------------------------------------------------------------------------------
def _raw(p, montgomery):
    """128 bytes of an affine point (None = infinity) in canonical or stored (Montgomery) form"""
    return GF.g2_bytes(p) if montgomery else SF.canonical_bytes(p)


@functools.lru_cache(maxsize=None)
def pool():
    """130 entries (name, canonical bytes, Montgomery bytes, expected status), shuffled with a fixed seed: generator multiples,
    random twist points outside the subgroup, points of order 10069 and 5864401, G2 + torsion sums, infinity, a coordinate equal
    to q (each of the four), a point off the twist.  The verdict of every point on the curve is Python's [r] P = O."""
    rnd = random.Random(401)
    by_class = {}
    for cls, p, member in SF.samples(3):
        by_class.setdefault(cls, []).append((p, member))
    outside = [(BP.twist_point_outside_subgroup(rnd), False) for _ in range(3)]
    gens = GF.G2.gen_muls([1, 2, R - 1] + [rnd.randrange(1, R) for _ in range(60)])
    g = GF.G2_GEN
    q_bytes = Q.to_bytes(32, "little")
    specials = [("infinity", bytes(128), bytes(128), VALID), ("off the twist", _raw(((1, 0), (1, 0)), False), _raw(((1, 0), (1, 0)), True), POINT)]
    for k in range(4):  # the generator with coordinate k replaced by q, which is not below q in either form
        specials.append(("coordinate %d is q" % k, *(b[:32 * k] + q_bytes + b[32 * k + 32:] for b in (_raw(g, False), _raw(g, True))), POINT))
    out = []
    for i in range(130):
        kind = i % 8
        if kind < 3:
            p = gens[i % len(gens)]
            out.append(("generator multiple", _raw(p, False), _raw(p, True), VALID if SF.in_g2_by_order(p) else SUBGROUP))
        elif kind == 7:
            out.append(specials[(i // 8) % len(specials)])
        else:
            cls = ("random_twist", "order_10069", "order_5864401", "g2_plus_torsion")[kind - 3]
            src = by_class[cls] + (outside if kind == 3 else [])
            p, member = src[(i // 8) % len(src)]
            if (i // 8) % 2:
                p = GF.G2.neg_aff(p)
            out.append((cls, _raw(p, False), _raw(p, True), VALID if member else SUBGROUP))
    rnd.shuffle(out)
    assert {e[3] for e in out[:63]} == {VALID, POINT, SUBGROUP}
    return tuple(out)


def statuses(raw, n, montgomery, method):
    import torch
    d = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).reshape(n, 128).copy()).cuda()
    out = PKG.bn254_g2_check_batch_device(d, montgomery=montgomery, method=method)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint32 and tuple(out.shape) == (n,)
    return [int(x) for x in out.cpu().numpy()]


# -- the aid -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_aid_against_python(n):
    """one point, a block less one, a block, a block and one, more than two blocks; both forms, both methods"""
    entries = pool()[:n] if n > 1 else [e for e in pool() if e[0] == "order_10069"][:1]
    want = [e[3] for e in entries]
    got = {}
    for montgomery in (False, True):
        raw = b"".join(e[2 if montgomery else 1] for e in entries)
        for method in ("fast", "order"):
            got[montgomery, method] = statuses(raw, n, montgomery, method)
            bad = [(i, entries[i][0], g, w) for i, (g, w) in enumerate(zip(got[montgomery, method], want)) if g != w]
            assert not bad, "montgomery %s, method %s: (index, class, got, want) %s" % (montgomery, method, bad[:6])
    assert got[False, "fast"] == got[False, "order"] == got[True, "fast"] == got[True, "order"]


def test_aid_on_each_class_alone():
    """one status per name, so that a criterion that misses one class is named: order 10069 is the one a sloppy test passes"""
    seen = {}
    for name, canonical, _, want in pool():
        seen.setdefault(name, (canonical, want))
    assert {"generator multiple", "random_twist", "order_10069", "order_5864401", "g2_plus_torsion", "infinity", "off the twist"} <= set(seen)
    names = sorted(seen)
    got = statuses(b"".join(seen[k][0] for k in names), len(names), False, "fast")
    assert dict(zip(names, got)) == {k: seen[k][1] for k in names}


def test_aid_empty_and_arguments():
    import torch
    out = PKG.bn254_g2_check_batch_device(torch.zeros((0, 128), dtype=torch.uint8, device="cuda"))
    assert out.dtype == torch.uint32 and tuple(out.shape) == (0,) and out.is_cuda
    with pytest.raises(PKG.WitnessCalcError, match="method must be one of"):
        PKG.bn254_g2_check_batch_device(torch.zeros((1, 128), dtype=torch.uint8, device="cuda"), method="slow")


# -- zkey --------------------------------------------------------------------------------------------------------------------------
def zkey_section(zkey, want):
    """(offset, size) of section `want`'s body"""
    off = 12
    for _ in range(struct.unpack_from("<I", zkey, 8)[0]):
        sid, size = struct.unpack_from("<IQ", zkey, off)
        off += 12
        if sid == want:
            return off, size
        off += size
    raise KeyError(want)


def with_b2(zkey, changes):
    """the key with the B2 points at the given indices replaced (affine points)"""
    off, _ = zkey_section(zkey, 7)
    z = bytearray(zkey)
    for i, p in changes.items():
        z[off + 128 * i:off + 128 * i + 128] = GF.g2_bytes(p)
    return bytes(z)


HEADER_G2 = {"beta2": 84 + 128, "gamma2": 84 + 256, "delta2": 84 + 448}


def with_header(zkey, changes):
    off, _ = zkey_section(zkey, 2)
    z = bytearray(zkey)
    for name, p in changes.items():
        z[off + HEADER_G2[name]:off + HEADER_G2[name] + 128] = GF.g2_bytes(p)
    return bytes(z)


@functools.lru_cache(maxsize=None)
def known_key(n_vars):
    return GF.KnownLog(n_vars, 1, 4, seed=n_vars).zkey


def bad_point(cls="random_twist", k=0):
    return [p for c, p, m in SF.samples(3) if c == cls and not m][k]


def _small_system(n_constraints=5):
    rnd = random.Random(31)
    shapes = [{"a": rnd.randrange(1, 4), "b": rnd.randrange(1, 4), "c": rnd.randrange(0, 3)} for _ in range(n_constraints)]
    pl = F.planted_system(rnd, 4, shapes, [1, R - 1, 2, None])
    return pl, F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=0)


@functools.lru_cache(maxsize=None)
def small_ptau(power, prepared=False):
    return PF.sections(power, TAU, ALPHA, BETA, prepared=prepared, points=device_points)


def device_points(group, scalars):
    """ptau_fixtures' `points` from the device's fixed-base multiplication (as tests/test_gpu_groth16_setup_ptau.py)"""
    import torch
    arr = np.frombuffer(b"".join((k % R).to_bytes(32, "little") for k in scalars), dtype=np.uint8).reshape(len(scalars), 32)
    raw = PKG.bn254_gen_mul_batch_device(torch.from_numpy(arr.copy()).cuda(), group)
    torch.cuda.synchronize()
    raw = raw.cpu().numpy().tobytes()
    return b"".join(GF.lem(int.from_bytes(raw[o:o + 32], "little")) for o in range(0, len(raw), 32))


@pytest.mark.parametrize("n_vars", (5, 70))
def test_untouched_keys_pass(n_vars):
    g = PKG.Groth16(known_key(n_vars), check_g2=True)
    g.check_g2()
    assert g.info["n_vars"] == n_vars


def test_keys_made_here_pass():
    pl, data = _small_system()
    r1 = PKG.R1cs(data)
    p = r1.qap_info()["domain_power"]
    PKG.Groth16(PKG.groth16_setup(r1, (TAU, ALPHA, BETA, 1, DELTA)), check_g2=True)
    PKG.Groth16(PKG.groth16_setup_ptau(r1, PF.assemble(small_ptau(p + 1)), DELTA), check_g2=True)
    PKG.Groth16.setup(r1).check_g2()


@pytest.mark.parametrize("n_vars", (5, 70))
def test_b2_offenders_are_named_with_index_and_count(n_vars, monkeypatch):
    key, last = known_key(n_vars), n_vars - 1
    cases = (({0: bad_point()}, 0, 1), ({last: bad_point()}, last, 1), ({last: bad_point(), 2: bad_point("g2_plus_torsion")}, 2, 2),
             ({3: bad_point("order_10069")}, 3, 1), ({1: bad_point("order_5864401"), 3: bad_point("order_10069", 1), last: bad_point(k=1)}, 1, 3))
    for chunk in (None, "24", "3"):  # the whole section at once; pieces of 24 (three for 70 points); pieces of 3
        if chunk is None:
            monkeypatch.delenv("CWC_G2_CHECK_CHUNK", raising=False)
        else:
            monkeypatch.setenv("CWC_G2_CHECK_CHUNK", chunk)
        for changes, first, count in cases:
            g = PKG.Groth16(with_b2(key, changes))  # without the flag the key loads, as before
            with pytest.raises(PKG.WitnessCalcError) as e:
                g.check_g2()
            assert str(e.value) == "zkey: section 7 (B2) point %d %s (%d of %d points are not)" % (first, SUB, count, n_vars)
            with pytest.raises(PKG.WitnessCalcError, match=r"section 7 \(B2\) point %d " % first):
                PKG.Groth16(with_b2(key, changes), check_g2=True)
        PKG.Groth16(with_b2(key, {1: None, last: GF.G2.gen_muls([7])[0]}), check_g2=True)  # infinity and another G2 point pass


def test_header_points_are_named_in_order():
    key = known_key(5)
    bad, tors = bad_point(), bad_point("order_10069")
    for names in (("beta2",), ("gamma2",), ("delta2",), ("gamma2", "delta2"), ("beta2", "delta2"), ("beta2", "gamma2", "delta2")):
        z = with_header(key, {n: (tors if n == "gamma2" else bad) for n in names})
        with pytest.raises(PKG.WitnessCalcError) as e:
            PKG.Groth16(z).check_g2()
        assert str(e.value) == "zkey: %s %s" % (names[0], SUB)
    # a header point before any B2 point
    z = with_b2(with_header(key, {"delta2": bad}), {0: bad})
    with pytest.raises(PKG.WitnessCalcError, match="^zkey: delta2 " + SUB):
        PKG.Groth16(z, check_g2=True)


def test_check_leaves_the_prover_alone():
    """check_g2 before and after a prove call: the proofs of fixed (r, s) do not change, and the check still passes"""
    pl, data = _small_system()
    r1 = PKG.R1cs(data)
    g = PKG.Groth16(PKG.groth16_setup(r1, (TAU, ALPHA, BETA, 1, DELTA)))
    ws = [pl.complete(random.Random(5 + i)) for i in range(3)]
    rows = F.rows_array(ws)
    rs = [(11 + i, 13 + i) for i in range(3)]
    g.check_g2()
    first = g.prove_batch(rows, rs)
    g.check_g2()
    assert np.array_equal(first, g.prove_batch(rows, rs))
    assert list(g.verifying_key().verify_batch(first, [w[1:2] for w in ws])) == [VALID] * 3


# -- ptau --------------------------------------------------------------------------------------------------------------------------
def swapped(power, prepared, sid, index, point):
    """the file with G2 point `index` of section `sid` replaced"""
    s = dict(small_ptau(power, prepared))
    raw = GF.g2_bytes(point) if not isinstance(point, bytes) else point
    s[sid] = s[sid][:128 * index] + raw + s[sid][128 * index + 128:]
    return PF.assemble(s)


@pytest.mark.parametrize("power", (3, 7))
def test_clean_files_pass(power):
    p = power - 1
    plain, prepared = PF.assemble(small_ptau(power)), PF.assemble(small_ptau(power, True))
    for mode in ("auto", "compute"):
        PKG.ptau_check_g2(plain, p, mode)
    for mode in ("auto", "file", "compute"):
        PKG.ptau_check_g2(prepared, p, mode)
    PKG.ptau_check_g2(prepared, 1, "file")
    with pytest.raises(PKG.WitnessCalcError, match="no prepared sections"):
        PKG.ptau_check_g2(plain, p, "file")


@pytest.mark.parametrize("power,chunk", ((3, None), (7, None), (7, "24")))
def test_swapped_points_are_found_where_they_are_read(power, chunk, monkeypatch):
    if chunk:
        monkeypatch.setenv("CWC_G2_CHECK_CHUNK", chunk)
    else:
        monkeypatch.delenv("CWC_G2_CHECK_CHUNK", raising=False)
    p, n = power - 1, 1 << (power - 1)
    bad, tors = bad_point(), bad_point("order_10069")

    def refused(data, mode, sid, name, index):
        with pytest.raises(PKG.WitnessCalcError) as e:
            PKG.ptau_check_g2(data, p, mode)
        assert str(e.value) == "ptau: section %d (%s) point %d %s" % (sid, name, index, SUB)

    # tauG2: read up to n - 1 when the Lagrange forms are computed, point 0 alone when they come from the file
    for i, pt in ((1, bad), (n - 1, tors), (n // 2 + 1, bad)):
        data = swapped(power, True, 3, i, pt)
        refused(data, "compute", 3, "tauG2", i)
        for mode in ("file", "auto"):
            PKG.ptau_check_g2(data, p, mode)
    refused(swapped(power, False, 3, n - 1, bad), "auto", 3, "tauG2", n - 1)
    for i in (n, 2 * n - 1):
        for mode in ("auto", "compute", "file"):
            PKG.ptau_check_g2(swapped(power, True, 3, i, bad), p, mode)
    # the smallest of two
    s = dict(small_ptau(power, True))
    s[3] = s[3][:128 * 2] + GF.g2_bytes(bad) + s[3][128 * 3:128 * (n - 1)] + GF.g2_bytes(tors) + s[3][128 * n:]
    refused(PF.assemble(s), "compute", 3, "tauG2", 2)
    # the Lagrange points of level p (from point n - 1 of section 13)
    for j, pt in ((0, bad), (n - 1, tors), (n // 2, bad)):
        data = swapped(power, True, 13, n - 1 + j, pt)
        for mode in ("file", "auto"):
            refused(data, mode, 13, "lagrange tauG2", n - 1 + j)
        PKG.ptau_check_g2(data, p, "compute")
    for i in (n - 2, 2 * n - 1):  # the levels next to it
        PKG.ptau_check_g2(swapped(power, True, 13, i, bad), p, "file")
    # betaG2, in every mode; before any other point
    for prepared, mode in ((False, "auto"), (True, "file"), (True, "compute")):
        refused(swapped(power, prepared, 6, 0, tors), mode, 6, "betaG2", 0)
    s = dict(small_ptau(power, True))
    s[6], s[3] = GF.g2_bytes(bad), s[3][:128] + GF.g2_bytes(bad) + s[3][256:]
    refused(PF.assemble(s), "compute", 6, "betaG2", 0)
    # a point off the curve among them is named as the host check names it
    off = GF.lem(1) + GF.lem(0) + GF.lem(1) + GF.lem(0)
    for fault in (off, GF.g2_bytes(GF.G2_GEN)[:96] + Q.to_bytes(32, "little")):
        data = swapped(power, True, 3, n - 1, fault)
        with pytest.raises(PKG.WitnessCalcError) as host:
            PKG.ptau_check(data, p, "compute")
        with pytest.raises(PKG.WitnessCalcError) as dev:
            PKG.ptau_check_g2(data, p, "compute")
        assert str(dev.value) == str(host.value) and "section 3 (tauG2) point %d" % (n - 1) in str(dev.value)


def test_setup_with_the_flag_refuses_and_without_it_is_unchanged():
    pl, data = _small_system()
    r1 = PKG.R1cs(data)
    p = r1.qap_info()["domain_power"]
    assert p == 3
    clean = PF.assemble(small_ptau(4, True))
    want = PKG.groth16_setup(r1, (TAU, ALPHA, BETA, 1, DELTA))
    for mode in ("auto", "file", "compute"):
        assert PKG.groth16_setup_ptau(r1, clean, DELTA, mode) == want
        assert PKG.groth16_setup_ptau(r1, clean, DELTA, mode, check_g2=True) == want
    bad = swapped(4, True, 3, 5, bad_point("order_10069"))
    with pytest.raises(PKG.WitnessCalcError) as direct:
        PKG.ptau_check_g2(bad, p, "compute")
    with pytest.raises(PKG.WitnessCalcError) as e:
        PKG.groth16_setup_ptau(r1, bad, DELTA, "compute", check_g2=True)
    assert str(e.value) == str(direct.value) == "ptau: section 3 (tauG2) point 5 " + SUB
    with pytest.raises(PKG.WitnessCalcError, match=r"section 3 \(tauG2\) point 5 " + SUB):
        PKG.Groth16.setup_ptau(r1, bad, DELTA, "compute", check_g2=True)
    assert PKG.groth16_setup_ptau(r1, bad, DELTA, "file", check_g2=True) == want  # not read under `file`
    # without the flag the file is taken as before, and the component of order 10069 ends up in B2
    key = PKG.groth16_setup_ptau(r1, bad, DELTA, "compute")
    assert key != want and len(key) == len(want)
    with pytest.raises(PKG.WitnessCalcError, match=r"section 7 \(B2\) point \d+ " + SUB):
        PKG.Groth16(key, check_g2=True)


# -- CLIs --------------------------------------------------------------------------------------------------------------------------
def _wtns(w):
    img = b"wtns" + struct.pack("<II", 2, 2) + struct.pack("<IQI", 1, 40, 32) + R.to_bytes(32, "little") + struct.pack("<I", len(w))
    return img + struct.pack("<IQ", 2, 32 * len(w)) + b"".join(x.to_bytes(32, "little") for x in w)


def _cli(name, *args):
    return subprocess.run([os.path.join(BIN, name)] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_cli_setup_check_g2(tmp_path):
    pl, data = _small_system()
    names = ("c.r1cs", "good.ptau", "bad.ptau", "d.txt", "a.zkey", "b.zkey", "c.zkey")
    c, good, bad, d, za, zb, zc = (tmp_path / n for n in names)
    c.write_bytes(data)
    good.write_bytes(PF.assemble(small_ptau(4)))
    bad.write_bytes(swapped(4, False, 3, 6, bad_point()))
    d.write_text("%d\n" % DELTA)
    p = _cli("groth16-setup", "--ptau", good, "--delta", d, c, za)
    assert p.returncode == 0, p
    p = _cli("groth16-setup", "--ptau", good, "--check-g2", "--delta", d, c, zb)
    assert p.returncode == 0, p
    assert za.read_bytes() == zb.read_bytes() == PKG.groth16_setup(PKG.R1cs(data), (TAU, ALPHA, BETA, 1, DELTA))
    p = _cli("groth16-setup", "--ptau", bad, "--delta", d, "--check-g2", c, zc)
    assert p.returncode == 2 and "ptau: section 3 (tauG2) point 6 " + SUB in p.stderr and not zc.exists(), p
    p = _cli("groth16-setup", "--ptau", bad, "--delta", d, c, zc)  # as before without the flag
    assert p.returncode == 0 and zc.exists(), p


def test_cli_prove_check_g2(tmp_path):
    import json
    pl, data = _small_system()
    w = pl.complete(random.Random(50))
    key = PKG.groth16_setup(PKG.R1cs(data), (TAU, ALPHA, BETA, 1, DELTA))
    c, z, zbad, wt = (tmp_path / n for n in ("c.r1cs", "c.zkey", "bad.zkey", "w.wtns"))
    c.write_bytes(data)
    z.write_bytes(key)
    zbad.write_bytes(with_b2(key, {2: bad_point("order_10069")}))
    wt.write_bytes(_wtns(w))
    vk = PKG.Groth16VerifyingKey.from_zkey(key)
    publics = []
    for tag, args in (("plain", (z, wt)), ("flag", ("--check-g2", z, wt)), ("r1cs", (c, z, wt)), ("r1cs_flag", (c, z, "--check-g2", wt))):
        proof, public = tmp_path / (tag + "_proof.json"), tmp_path / (tag + "_public.json")
        p = _cli("groth16-prove", *args, proof, public)
        assert p.returncode == 0, p
        publics.append(public.read_bytes())
        assert vk.verify(json.loads(proof.read_text()), json.loads(public.read_text()))  # (r and s are drawn: the proofs differ)
    assert len(set(publics)) == 1
    for args in (("--check-g2", zbad, wt), (c, zbad, wt, "--check-g2")):
        proof, public = tmp_path / "no_proof.json", tmp_path / "no_public.json"
        p = _cli("groth16-prove", *args, proof, public)
        assert p.returncode == 2 and "zkey: section 7 (B2) point 2 %s (1 of %d points are not)" % (SUB, pl.n_wires) in p.stderr, p
        assert not proof.exists() and not public.exists()
    p = _cli("groth16-prove", zbad, wt, tmp_path / "p.json", tmp_path / "q.json")  # as before without the flag
    assert p.returncode == 0, p
