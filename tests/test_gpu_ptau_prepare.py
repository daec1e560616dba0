"""The Lagrange sections 12 to 15 of a `.ptau` on an MI355X: ptau_prepare_phase2 writes them (r1cs/setup_ptau.hip's all-levels
transform), ptau_check_lagrange checks them against sections 2 to 5 (r1cs/contribute.hip: the 128-bit combination of the
Lagrange points against the full-width one of the monomial points).  Expected points are scalars times the generator: from the
plain-Python curve up to power 3, from the fixed-base table kernel (bn254_gen_mul_batch_device, independent of everything under
test) above that; affine points are unique, so every comparison is byte equality.  tests/ptau_fixtures.py writes the last level
of section 12 from the true tau, the library from the truncated input (T_0 .. T_{2n-2}, O): that one level is compared with
lag(power + 1, t + [0]) here and never with the fixture (test_ptau_prepare_host.py pins the definition in plain integers).

The stage kernel gives a wave one twiddle index while a launch's top level is at least six stages ahead (top - s >= 6) and
consecutive indices in the last five stages; stage 0 has k = 0 only, so power 7 (top levels 7 and 8) is the smallest file whose
launches have both kinds of stages with a multiplication."""
import functools
import math
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import cwc_import
from tests import g2_subgroup_fixtures as SF
from tests import groth16_fixtures as GF
from tests import ptau_fixtures as PF
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
R, Q = GF.R, GF.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "circom-witnesscalc_amd")
MONT_INV = pow(GF.MONT, -1, Q)
SEED = bytes(range(7, 39))
WIDTH = {12: 64, 13: 128, 14: 64, 15: 64}
NAME = {12: "lagrange tauG1", 13: "lagrange tauG2", 14: "lagrange alphaTauG1", 15: "lagrange betaTauG1"}

_rnd = random.Random(800)
TAU, ALPHA, BETA, TAU_OTHER, DELTA_RANDOM = (_rnd.randrange(2, R) for _ in range(5))

pytestmark = pytest.mark.gpu


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
def system(p):
    """the planted system of test_gpu_groth16_setup.py::power_case for the domain 2^p (construction restated):
    (constraints, public signals, `.r1cs` bytes, R1cs)"""
    n_pub_in = 0 if p <= 2 else 2
    n_pub = n_pub_in + (0 if p <= 2 else 1)
    n_c = (1 << p) - n_pub - 1 - random.Random(p).randrange(0, 1 << (p - 1))
    rnd = random.Random(100 + p)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(n_c)]
    pl = F.planted_system(rnd, 6, shapes, [1, R - 1, 2, F.MONT_R, None])
    data = F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=n_pub - n_pub_in, n_pub_in=n_pub_in)
    r1 = PKG.R1cs(data)
    assert r1.qap_info()["domain_power"] == p
    return pl.constraints, n_pub, data, r1


def points_for(power):
    return PF.python_points if power <= 3 else device_points


@functools.lru_cache(maxsize=None)
def file_sections(power, prepared=False, lagrange_tau=None, ceremony_power=None):
    return PF.sections(power, TAU, ALPHA, BETA, prepared=prepared, lagrange_tau=lagrange_tau, ceremony_power=ceremony_power, points=points_for(power))


@functools.lru_cache(maxsize=None)
def plain(power):
    return PF.assemble(file_sections(power))


@functools.lru_cache(maxsize=None)
def prepared(power):
    """the library's own output for the honest file"""
    return PKG.ptau_prepare_phase2(plain(power))


@functools.lru_cache(maxsize=None)
def truncated_top(power):
    """level power + 1 of section 12 as the library defines it: Lag of (T_0 .. T_{2n-2}, O)"""
    t = [pow(TAU, i, R) for i in range((2 << power) - 1)]
    return points_for(power)(1, PF.lag(power + 1, t + [0]))


def split(image):
    """`.ptau` bytes -> [(id, body)] in file order"""
    assert image[:4] == b"ptau" and struct.unpack_from("<I", image, 4)[0] == 1
    off, out = 12, []
    for _ in range(struct.unpack_from("<I", image, 8)[0]):
        sid, size = struct.unpack_from("<IQ", image, off)
        out.append((sid, image[off + 12:off + 12 + size]))
        off += 12 + size
    assert off == len(image)
    return out


def assert_lagrange_sections(image, power):
    """levels 0 .. power of sections 12 to 15 against the fixture, level power + 1 of section 12 against the truncated definition"""
    got, want, n = dict(split(image)[-4:]), file_sections(power, True), 1 << power
    assert [sid for sid, _ in split(image)[-4:]] == [12, 13, 14, 15]
    for sid in (13, 14, 15):
        assert got[sid] == want[sid], "section %d differs" % sid
    shared = 64 * (2 * n - 1)
    assert len(got[12]) == 64 * (4 * n - 1)
    assert got[12][:shared] == want[12][:shared], "section 12 differs below its last level"
    assert got[12][shared:] == truncated_top(power), "the last level of section 12 is not Lag of (T_0 .. T_{2n-2}, O)"


# -- 1. the bytes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", (0, 1, 2, 3, 5, 7))
def test_prepared_bytes(power):
    out = prepared(power)
    assert_lagrange_sections(out, power)
    assert split(out)[:-4] == split(plain(power))
    info = PKG.ptau_info(out)
    assert info["prepared"] and info["power"] == power and not PKG.ptau_info(plain(power))["prepared"]
    assert PKG.ptau_prepare_phase2(bytearray(plain(power))) == out


def test_prepared_in_small_pieces(monkeypatch):
    """CWC_CONTRIBUTE_CHUNK = 100: every section leaves the device in several pieces, the last one short"""
    monkeypatch.setenv("CWC_CONTRIBUTE_CHUNK", "100")
    assert PKG.ptau_prepare_phase2(plain(5)) == prepared(5)


def test_carried_sections_and_order():
    """an unknown section between the known ones, a shuffled order and a ceremony power above the file's: all carried as they are"""
    secs = dict(file_sections(3, ceremony_power=11))
    secs[40] = b"not a section this library knows"
    order = [3, 40, 1, 7, 5, 2, 6, 4]
    out = PKG.ptau_prepare_phase2(PF.assemble(secs, order=order))
    assert split(out)[:-4] == [(sid, secs[sid]) for sid in order]
    assert_lagrange_sections(out, 3)
    info = PKG.ptau_info(out)
    assert info["prepared"] and info["ceremony_power"] == 11 and info["power"] == 3


def test_prepared_sections_are_replaced():
    """an input whose sections 12 to 15 were written from another tau comes out right, whatever their place in the file"""
    wrong = dict(file_sections(3, True, TAU_OTHER))
    assert wrong[14] != file_sections(3, True)[14]
    assert PKG.ptau_prepare_phase2(PF.assemble(wrong)) == prepared(3)
    assert PKG.ptau_prepare_phase2(PF.assemble(wrong, order=[12, 1, 2, 13, 3, 4, 5, 15, 6, 7, 14])) == prepared(3)


def test_prepare_names_a_point_fault():
    """a monomial point off its curve, and one with a coordinate >= q, in the words of the setup's own check"""
    secs = file_sections(3)
    for sid, width, index, fault, pattern in ((2, 64, 14, GF.lem(1) + GF.lem(3), r"section 2 \(tauG1\) point 14 is not on the G1 curve"),
                                              (3, 128, 5, bytes(32) + Q.to_bytes(32, "little") + bytes(64), r"section 3 \(tauG2\) point 5 has a coordinate >= q"),
                                              (5, 64, 7, GF.lem(1) + GF.lem(3), r"section 5 \(betaTauG1\) point 7 is not on the G1 curve")):
        bad = dict(secs)
        bad[sid] = secs[sid][:width * index] + fault + secs[sid][width * (index + 1):]
        with pytest.raises(PKG.WitnessCalcError, match=pattern):
            PKG.ptau_prepare_phase2(PF.assemble(bad))


# -- 2. it feeds the setup ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", (3, 4))
def test_prepared_file_feeds_the_setup(p):
    """power 5, domains 2^3 and 2^4: the key read from the prepared file is the key computed from the plain one"""
    r1 = system(p)[3]
    assert PKG.groth16_setup_ptau(r1, prepared(5), DELTA_RANDOM, "file") == PKG.groth16_setup_ptau(r1, plain(5), DELTA_RANDOM, "compute")


# -- 3. the check ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", (1, 3, 5, 7))
def test_check_accepts_the_prepared_file(power):
    for seed in (SEED, bytes(32), None):
        PKG.ptau_check_lagrange(prepared(power), seed=seed)
    for p in range(power):
        PKG.ptau_check_lagrange(prepared(power), p, seed=SEED)
    PKG.ptau_check_lagrange(bytearray(prepared(power)), power - 1)


def test_check_of_a_file_of_power_0():
    PKG.ptau_check_lagrange(prepared(0), seed=SEED)
    with pytest.raises(PKG.WitnessCalcError, match="needs a ceremony of power 1 or more"):
        PKG.ptau_check_lagrange(prepared(0), 0)


@pytest.mark.parametrize("power", (3, 7))
def test_check_and_the_fixtures_last_level(power):
    """the fixture writes level power + 1 of section 12 from the true tau: no setup reads it, so every domain passes, and the
    all-level check names section 12 and that level"""
    fixture = PF.assemble(file_sections(power, True))
    for p in range(power):
        PKG.ptau_check_lagrange(fixture, p, seed=SEED)
    with pytest.raises(PKG.WitnessCalcError, match=r"^ptau: section 12 \(lagrange tauG1\) does not hold the Lagrange forms of section 2: level %d is the first" % (power + 1)):
        PKG.ptau_check_lagrange(fixture, seed=SEED)


def test_check_in_small_pieces(monkeypatch):
    monkeypatch.setenv("CWC_CONTRIBUTE_CHUNK", "100")
    PKG.ptau_check_lagrange(prepared(7), seed=SEED)
    PKG.ptau_check_lagrange(prepared(7), 6, seed=SEED)
    body = dict(split(prepared(7)))[14]
    with pytest.raises(PKG.WitnessCalcError, match=r"section 14 \(lagrange alphaTauG1\) level 6 does not hold"):
        PKG.ptau_check_lagrange(with_section(7, 14, body[:64 * 100] + body[64 * 99:64 * 100] + body[64 * 101:]), 6, seed=SEED)


def test_check_refusals_before_the_equations():
    with pytest.raises(PKG.WitnessCalcError, match="no prepared sections"):
        PKG.ptau_check_lagrange(plain(3))
    with pytest.raises(PKG.WitnessCalcError, match="no prepared sections"):
        PKG.ptau_check_lagrange(plain(3), 2)
    with pytest.raises(PKG.WitnessCalcError, match=r"domain 2\^3 needs a ceremony of power 4 or more, this file has power 3"):
        PKG.ptau_check_lagrange(prepared(3), 3)


def _fq(b):
    return int.from_bytes(b, "little") * MONT_INV % Q


def point_of(stored):
    if not any(stored):
        return None
    c = [_fq(stored[o:o + 32]) for o in range(0, len(stored), 32)]
    return (c[0], c[1]) if len(c) == 2 else ((c[0], c[1]), (c[2], c[3]))


def stored_of(curve, jac):
    return (GF.g1_bytes if curve is GF.G1 else GF.g2_bytes)(curve.to_affine(jac))


def with_section(power, sid, body):
    """the library's prepared file with the body of one section replaced"""
    secs = dict(split(prepared(power)))
    secs[sid] = body
    return PF.assemble(secs)


def level_faults(power, sid, m):
    """{name: (the prepared file with that fault in level m of section sid, what the message says after the section)}"""
    width, body, first = WIDTH[sid], dict(split(prepared(power)))[sid], (1 << m) - 1
    curve = GF.G2 if sid == 13 else GF.G1
    at = lambda k: width * (first + k)  # noqa: E731
    put = lambda k, new: with_section(power, sid, body[:at(k)] + new + body[at(k) + len(new):])  # noqa: E731
    k = (1 << m) - 1  # the level's last point
    here = body[at(k):at(k) + width]
    wrong = " does not hold the Lagrange forms of section %d" % (sid - 10)
    off_curve = GF.lem(1) + GF.lem(3) if width == 64 else GF.lem(1) + GF.lem(0) + GF.lem(1) + GF.lem(0)
    out = {"doubled": (put(k, stored_of(curve, curve.mul(point_of(here), 2))), wrong),
           "off_curve": (put(k, off_curve), r" point %d is not on the G%d curve" % (first + k, width // 64)),
           "coordinate": (put(k, here[:width - 32] + Q.to_bytes(32, "little")), r" point %d has a coordinate >= q" % (first + k))}
    if m >= 1:
        out["swapped"] = (put(k - 1, here + body[at(k - 1):at(k - 1) + width]), wrong)
        other = file_sections(power, True, TAU_OTHER)[sid][at(0):at(0) + (width << m)]
        assert other != body[at(0):at(0) + len(other)]
        out["another_tau"] = (put(0, other), wrong)
    if sid == 13:
        torsion = SF.exact_order(random.Random(900 + m), SF.SMALL[0])
        out["small_order"] = (put(k, stored_of(curve, curve.add(curve.jac(point_of(here)), curve.jac(torsion)))),
                              r" point %d is not in the order-r subgroup of G2" % (first + k))
    return out


@pytest.mark.parametrize("sid", (12, 13, 14, 15))
@pytest.mark.parametrize("power", (3, 7))
def test_check_refuses(power, sid):
    """levels 0, 1, power - 1 and the section's last: one point doubled, two swapped, the level of another tau, a point off the
    curve, a coordinate >= q and, in G2, a component of small order.  All-level mode names the section (and finds the level); the
    domain that reads the level names section and level; a domain that does not read it accepts the file."""
    top = power + 1 if sid == 12 else power
    who = r"^ptau: section %d \(%s\)" % (sid, NAME[sid])
    for m in (0, 1, power - 1, top):
        reader = m if m < power else m - 1 if sid == 12 and m == power else None  # the domain whose setup reads level m
        bystander = next(p for p in range(power) if p != m and not (sid == 12 and p + 1 == m))
        for name, (file, says) in level_faults(power, sid, m).items():
            is_equation = says.startswith(" does not hold")
            with pytest.raises(PKG.WitnessCalcError, match=who + (says + ": level %d is the first that does not$" % m if is_equation else says)):
                PKG.ptau_check_lagrange(file, seed=SEED)
            if reader is not None:
                with pytest.raises(PKG.WitnessCalcError, match=who + (" level %d" % m + says + "$" if is_equation else says)):
                    PKG.ptau_check_lagrange(file, reader, seed=SEED)
            PKG.ptau_check_lagrange(file, bystander, seed=SEED)  # (raises with the fault's name in the traceback's locals)


def test_check_with_a_drawn_seed_refuses_too():
    file, _ = level_faults(3, 14, 2)["doubled"]
    for _ in range(3):
        with pytest.raises(PKG.WitnessCalcError, match=r"section 14 \(lagrange alphaTauG1\) level 2 does not hold the Lagrange forms of section 4$"):
            PKG.ptau_check_lagrange(file, 2)


# -- 4. the full-width combination aids -----------------------------------------------------------------------------------------
EDGE_SCALARS = (0, 1, R - 1, 1 << 128, (1 << 128) - 1, 0x12345678 << 224)


def _canonical_bytes(p, group):
    if p is None:
        return bytes(64 * group)
    cs = p if group == 1 else (p[0][0], p[0][1], p[1][0], p[1][1])
    return b"".join(x.to_bytes(32, "little") for x in cs)


def _lincomb(group, logs, scalars, form):
    import torch
    pts = device_canonical(group, logs) if form == "canonical" else np.frombuffer(device_points(group, logs), dtype=np.uint8).reshape(len(logs), 64 * group)
    sc = np.frombuffer(b"".join(x.to_bytes(32, "little") for x in scalars), dtype=np.uint8).reshape(len(scalars), 32)
    call = PKG.bn254_g1_lincomb_device if group == 1 else PKG.bn254_g2_lincomb_device
    got = call(torch.from_numpy(pts.copy()).cuda(), torch.from_numpy(sc.copy()).cuda(), form=form)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (64 * group,)
    return got.cpu().numpy().tobytes()


def _expected(group, logs, scalars, form):
    curve = GF.G1 if group == 1 else GF.G2
    p = curve.gen_muls([sum(s * k for s, k in zip(scalars, logs)) % R])[0]
    if form == "canonical":
        return _canonical_bytes(p, group)
    return (GF.g1_bytes if group == 1 else GF.g2_bytes)(p)


@pytest.mark.parametrize("form", ("canonical", "montgomery"))
@pytest.mark.parametrize("group,n", [(1, n) for n in (1, 255, 256, 257, 513)] + [(2, n) for n in (1, 63, 64, 65, 129)])
def test_full_width_lincomb_aids(group, n, form):
    """the workgroup seams of both groups (256 threads in G1, one wave of 64 in G2).  From the second size on the list holds the
    scalars 0, 1, r - 1, 2^128, 2^128 - 1 and one with only its top word set, an infinity with a full-width scalar, and a pair
    P, -P with one scalar; with one point, every edge scalar in turn."""
    rnd = random.Random(4000 + 10 * n + group)
    if n == 1:
        k = rnd.randrange(1, R)
        for s in EDGE_SCALARS + (rnd.randrange(1 << 250, R),):
            assert _lincomb(group, [k], [s], form) == _expected(group, [k], [s], form), hex(s)
        assert _lincomb(group, [0], [R - 1], form) == bytes(64 * group)
        return
    logs = [rnd.randrange(1, R) for _ in range(n)]
    scalars = [rnd.randrange(R) for _ in range(n)]
    scalars[:len(EDGE_SCALARS)] = EDGE_SCALARS
    logs[9] = 0                                           # infinity among the points
    logs[11 + 32], scalars[11 + 32] = R - logs[11], scalars[11]  # P and -P with one scalar
    scalars[n - 1] = R - 1
    want = _expected(group, logs, scalars, form)
    assert any(want) and _lincomb(group, logs, scalars, form) == want


def test_full_width_lincomb_aid_arguments():
    import torch
    pts, sc = torch.zeros((3, 64), dtype=torch.uint8, device="cuda"), torch.zeros((3, 32), dtype=torch.uint8, device="cuda")
    assert not PKG.bn254_g1_lincomb_device(pts, sc).cpu().numpy().any()
    with pytest.raises(PKG.WitnessCalcError, match="form must be"):
        PKG.bn254_g1_lincomb_device(pts, sc, form="jacobian")


# -- 5. the key check -----------------------------------------------------------------------------------------------------------
def test_verify_key_with_check_lagrange():
    """p4 (domain 2^4) on a prepared file of power 5.  The honest triple passes with the flag.  A file whose level 4 of section 15
    holds one foreign point is refused with the Lagrange message when the flag is set; without the flag the same call PASSES
    today: the point sits at domain index 15, this system uses the indices 0 .. 12 only (9 constraints and the 4 rows of the
    public wires), so the remade key never reads it."""
    cons, n_pub, _, r1 = system(4)
    assert len(cons) + n_pub + 1 <= 15
    key = PKG.groth16_setup_ptau(r1, plain(5), 1, "compute")
    assert PKG.groth16_verify_key(key, r1, prepared(5), lagrange="file", check_lagrange=True, seed=SEED) == []
    assert PKG.groth16_verify_key(key, r1, prepared(5), lagrange="auto", check_lagrange=True, seed=SEED) == []
    assert PKG.groth16_verify_key(key, r1, plain(5), lagrange="auto", check_lagrange=True, seed=SEED) == []  # nothing prepared: nothing to check
    body = dict(split(prepared(5)))[15]
    at = 64 * ((1 << 4) - 1 + 15)
    foreign = with_section(5, 15, body[:at] + device_points(1, [12345]) + body[at + 64:])
    with pytest.raises(PKG.WitnessCalcError, match=r"^ptau: section 15 \(lagrange betaTauG1\) level 4 does not hold the Lagrange forms of section 5$"):
        PKG.groth16_verify_key(key, r1, foreign, lagrange="file", check_lagrange=True, seed=SEED)
    assert PKG.groth16_verify_key(key, r1, foreign, lagrange="file", seed=SEED) == []
    assert PKG.groth16_verify_key(key, r1, foreign, lagrange="compute", check_lagrange=True, seed=SEED) == []  # compute does not read them


# -- 6. the CLI and the timers --------------------------------------------------------------------------------------------------
def test_cli_chain(tmp_path):
    """groth16-setup --prepare-ptau, --check-lagrange in both modes, --ptau ... --lagrange file on the result, and
    groth16-contribute --verify-key --check-lagrange, at power 3"""
    r1cs_bytes = system(2)[2]
    path = lambda name: str(tmp_path / name)  # noqa: E731
    (tmp_path / "in.ptau").write_bytes(plain(3))
    (tmp_path / "c.r1cs").write_bytes(r1cs_bytes)
    (tmp_path / "d.txt").write_text("1\n")
    setup = os.path.join(BIN, "groth16-setup")
    run = lambda *args: subprocess.run(list(args), capture_output=True, text=True, timeout=300)  # noqa: E731
    p = run(setup, "--prepare-ptau", path("in.ptau"), path("out.ptau"))
    assert p.returncode == 0 and p.stdout == "" and p.stderr == "", p
    assert (tmp_path / "out.ptau").read_bytes() == prepared(3)
    for extra in ((), ("--domain-power", "2")):
        p = run(setup, "--check-lagrange", *extra, path("out.ptau"))
        assert p.returncode == 0 and p.stdout == "OK!\n", p
    p = run(setup, "--check-lagrange", path("in.ptau"))
    assert p.returncode == 2 and "no prepared sections" in p.stderr and p.stdout == "", p
    file, _ = level_faults(3, 14, 2)["doubled"]
    (tmp_path / "bad.ptau").write_bytes(file)
    p = run(setup, "--check-lagrange", "--domain-power", "2", path("bad.ptau"))
    assert p.returncode == 1 and "section 14 (lagrange alphaTauG1) level 2 does not hold the Lagrange forms of section 4" in p.stderr, p
    p = run(setup, "--ptau", path("out.ptau"), "--lagrange", "file", "--delta", path("d.txt"), path("c.r1cs"), path("c.zkey"))
    assert p.returncode == 0, p
    assert (tmp_path / "c.zkey").read_bytes() == PKG.groth16_setup_ptau(system(2)[3], plain(3), 1, "compute")
    contribute = os.path.join(BIN, "groth16-contribute")
    p = run(contribute, "--verify-key", "--lagrange", "file", "--check-lagrange", path("c.r1cs"), path("out.ptau"), path("c.zkey"))
    assert p.returncode == 0 and p.stdout.startswith("OK!"), p
    p = run(contribute, "--verify-key", "--lagrange", "file", "--check-lagrange", path("c.r1cs"), path("bad.ptau"), path("c.zkey"))
    assert p.returncode == 1 and "INVALID: ptau: section 14 (lagrange alphaTauG1) level 2" in p.stderr, p


def test_phase_timer():
    PKG.ptau_prepare_phase2(plain(5))
    ms = PKG.ptau_prepare_phase_ms()
    assert list(ms) == ["load", "idft_g1", "idft_g2", "affine"] == list(PKG.PTAU_PREPARE_PHASES)
    assert all(math.isfinite(x) and x > 0 for x in ms.values()), ms
