"""G2 subgroup membership without a device: the psi criterion restated in Python (tests/g2_subgroup_fixtures.py) against
[r] P = O on the six point classes; the host build of r1cs/g2_subgroup_gfx950.hpp (a stand-alone program under
-fsanitize=address,undefined) against the same verdicts, and its g2_psi on projective XYZZ input against psi of the affine
point; and what gwb_bn254_g2_check_batch_device, gwb_zkey_check_g2 and gwb_ptau_check_g2 refuse before they reach a device,
the `.ptau` refusals with gwb_ptau_check's own messages; the CLIs' --check-g2 usage errors."""
import ctypes
import functools
import os
import random
import struct
import subprocess

import pytest

import cwc_import
from tests import g2_subgroup_fixtures as SF
from tests import groth16_fixtures as GF
from tests import ptau_fixtures as PF
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
Q, R = GF.Q, GF.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "circom-witnesscalc_amd")
PER_CLASS = 4
IN_G2 = {"random_twist": False, "cofactor_cleared": True, "order_10069": False, "order_5864401": False, "g2_plus_torsion": False,
         "r_times": False}


# -- the criterion in Python -----------------------------------------------------------------------------------------------------
def test_psi_is_an_endomorphism_of_the_twist_and_is_q_on_g2():
    rnd = random.Random(11)
    p, q = SF.random_twist_point(rnd), SF.random_twist_point(rnd)
    assert GF.G2.on_curve(SF.psi(p))
    s = GF.G2.to_affine(GF.G2.add(GF.G2.jac(p), GF.G2.jac(q)))
    assert SF.psi(s) == GF.G2.to_affine(GF.G2.add(GF.G2.jac(SF.psi(p)), GF.G2.jac(SF.psi(q))))
    g = GF.G2.gen_muls([rnd.randrange(1, R)])[0]
    assert SF.psi(g) == GF.G2.to_affine(GF.G2.mul(g, Q % R))


def test_classes_are_what_their_names_say():
    for cls, p, member in SF.samples(PER_CLASS):
        assert GF.G2.on_curve(p)
        assert member == IN_G2[cls], cls  # ([r] P of a random point has its order in c2: outside G2 unless it is O)
        if cls.startswith("order_"):
            assert p is not None and GF.G2.is_inf(GF.G2.mul(p, int(cls[6:])))
    assert any(m for _, _, m in SF.samples(PER_CLASS)) and not all(m for _, _, m in SF.samples(PER_CLASS))


def test_python_criterion_agrees_with_multiplication_by_r():
    for cls, p, member in SF.samples(PER_CLASS):
        assert SF.in_g2_by_psi(p) == member, cls
        assert SF.in_g2_by_psi_short(p) == member, cls
    assert SF.in_g2_by_psi(None) and SF.in_g2_by_psi(GF.G2_GEN)


# -- the header on the host ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("g2_subgroup_host") / "g2_subgroup_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "g2_subgroup_host.cc")])
    return exe


def run_host(exe, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.split("\n")[:-1]


def hx(v):
    return "%064x" % v


def point_words(p):
    return "%s %s %s %s" % ((hx(0),) * 4 if p is None else (hx(p[0][0]), hx(p[0][1]), hx(p[1][0]), hx(p[1][1])))


def test_host_verdicts_equal_pythons(host_program):
    pts = [(cls, p, m) for cls, p, m in SF.samples(PER_CLASS)] + [("infinity", None, True), ("generator", GF.G2_GEN, True),
                                                                  ("minus generator", GF.G2.neg_aff(GF.G2_GEN), True)]
    got = run_host(host_program, ["S " + point_words(p) for _, p, _ in pts])
    assert len(got) == len(pts)
    for (cls, _, member), line in zip(pts, got):
        want = "S %d %d 1" % (member, member)
        assert line == want, (cls, line, want)
    assert {m for _, _, m in pts} == {True, False}


def test_host_psi_on_projective_input(host_program):
    rnd = random.Random(12)
    pts = [p for _, p, _ in SF.samples(PER_CLASS)[::3] if p is not None] + [GF.G2_GEN]
    lam = [(rnd.randrange(1, Q), rnd.randrange(Q)) for _ in pts]
    lam[0], lam[1] = (1, 0), (0, rnd.randrange(1, Q))
    got = run_host(host_program, ["P %s %s %s" % (point_words(p), hx(l[0]), hx(l[1])) for p, l in zip(pts, lam)])
    for p, line in zip(pts, got):
        assert line == "P " + point_words(SF.psi(p))


# -- argument errors, no device --------------------------------------------------------------------------------------------------
def _call(name, *args):
    st = PKG.GwStatus()
    rc = getattr(PKG.r1cs_lib(), name)(*args, ctypes.byref(st))
    msg = ctypes.string_at(st.error_msg).decode() if st.error_msg else ""
    if st.error_msg:
        PKG._libc.free(st.error_msg)
    return rc, msg


def test_aid_refuses_form_and_method_before_the_device():
    buf = ctypes.create_string_buffer(128)
    out = ctypes.create_string_buffer(4)
    assert _call("gwb_bn254_g2_check_batch_device", buf, 1, 2, 0, out, None) == (1, "gwb_bn254_g2_check_batch_device: unknown form 2")
    rc, msg = _call("gwb_bn254_g2_check_batch_device", buf, 1, 0, 2, out, None)
    assert rc == 1 and msg.startswith("gwb_bn254_g2_check_batch_device: unknown method 2")
    assert _call("gwb_bn254_g2_check_batch_device", None, 1, 0, 0, out, None) == (1, "gwb_bn254_g2_check_batch_device: NULL argument")
    assert _call("gwb_bn254_g2_check_batch_device", None, 0, 1, 1, None, None) == (0, "")  # n = 0: nothing to do
    assert _call("gwb_zkey_check_g2", None) == (1, "gwb_zkey_check_g2: NULL argument")
    with pytest.raises(PKG.WitnessCalcError, match="method must be one of"):
        PKG.bn254_g2_check_batch_device(None, method="slow")


TAU, ALPHA, BETA = 0x1234567, 0x89abcd, 0xfedcba9
POWER = 3


@functools.lru_cache(maxsize=None)
def secs(prepared=False):
    return PF.sections(POWER, TAU, ALPHA, BETA, prepared=prepared)


def broken(prepared=False, **changes):
    s = dict(secs(prepared))
    for k, v in changes.items():
        s[int(k[1:])] = v
    return PF.assemble(s)


def patched(body, at, new):
    return body[:at] + new + body[at + len(new):]


def test_ptau_refusals_are_gwb_ptau_checks_and_need_no_device():
    """parse, plan and the header points: the message of ptau_check_g2 is ptau_check's, on a machine without a GPU"""
    good, s = PF.assemble(secs()), secs()
    off_g2 = GF.lem(1) + GF.lem(0) + GF.lem(1) + GF.lem(0)
    cases = ((b"ptaw" + good[4:], 2, "auto"), (good[:-1], 2, "auto"), (good[:12] + good[12:20], 2, "auto"), (good + b"\0", 2, "auto"),
             (good, 3, "auto"), (good, 9, "compute"), (good, 2, "file"),
             (broken(s3=s[3][:-128]), 2, "auto"), (broken(s1=PF.header(29)), 2, "auto"),
             (broken(s6=patched(s[6], 0, off_g2)), 2, "compute"), (broken(s6=patched(s[6], 96, Q.to_bytes(32, "little"))), 2, "compute"),
             (broken(s4=patched(s[4], 0, GF.lem(1) + GF.lem(3))), 2, "compute"), (broken(s5=patched(s[5], 32, Q.to_bytes(32, "little"))), 1, "auto"),
             (broken(s3=patched(s[3], 0, GF.g2_bytes(GF.G2.gen_muls([2])[0]))), 2, "auto"))
    for data, p, mode in cases:
        with pytest.raises(PKG.WitnessCalcError) as want:
            PKG.ptau_check(data, p, mode)
        with pytest.raises(PKG.WitnessCalcError) as got:
            PKG.ptau_check_g2(data, p, mode)
        assert str(got.value) == str(want.value) and str(got.value).startswith("ptau: ")
    with pytest.raises(PKG.WitnessCalcError, match="truncated section 7"):
        PKG.ptau_check_g2(good[:-1], 2)
    with pytest.raises(PKG.WitnessCalcError, match=r"domain 2\^3 needs a ceremony of power 4 or more, this file has power 3"):
        PKG.ptau_check_g2(good, 3)
    with pytest.raises(PKG.WitnessCalcError, match="lagrange must be one of"):
        PKG.ptau_check_g2(good, 2, "lazy")
    assert _call("gwb_ptau_check_g2", None, 5, 2, 0) == (1, "gwb_ptau_check_g2: NULL argument")
    rc, msg = _call("gwb_ptau_check_g2", good, len(good), 2, 3)
    assert rc == 1 and msg.startswith("ptau: lagrange mode 3")


def test_setup_with_check_g2_refuses_on_the_host_first():
    rnd = random.Random(31)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(5)]
    pl = F.planted_system(rnd, 4, shapes, [1, R - 1, 2, None])
    r3 = PKG.R1cs(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=0))
    assert r3.qap_info()["domain_power"] == 3
    for kw in ({}, {"check_g2": True}):
        with pytest.raises(PKG.WitnessCalcError, match=r"needs a ceremony of power 4"):
            PKG.groth16_setup_ptau(r3, PF.assemble(secs()), 1, **kw)
    with pytest.raises(PKG.WitnessCalcError, match=r"needs a ceremony of power 4"):
        PKG.Groth16.setup_ptau(r3, PF.assemble(secs()), 1, check_g2=True)


# -- the CLIs' flag, as far as no device is needed -------------------------------------------------------------------------------
def _cli(name, *args):
    return subprocess.run([os.path.join(BIN, name)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_cli_setup_check_g2_usage(tmp_path):
    c, z, pt, t = (tmp_path / n for n in ("c.r1cs", "c.zkey", "pot.ptau", "t.txt"))
    rnd = random.Random(31)
    pl = F.planted_system(rnd, 4, [{"a": 1, "b": 1, "c": 1}] * 5, [1, R - 1, 2, None])
    c.write_bytes(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=0))
    pt.write_bytes(PF.assemble(secs()))
    t.write_text("5 7 11 13 17\n")
    for args in (("--check-g2", c, z), ("--trapdoor", t, "--check-g2", c, z), ("--ptau", pt, "--check-g2", "--check-g2", c, z)):
        p = _cli("groth16-setup", *args)
        assert p.returncode == 2 and "usage" in p.stderr and "--check-g2" in p.stderr, (args, p)
    # the file's refusals come before the device: a domain the file cannot serve
    p = _cli("groth16-setup", "--ptau", pt, "--check-g2", c, z)
    assert p.returncode == 2 and "needs a ceremony of power 4" in p.stderr, p
    assert not z.exists()


def _wtns(w):
    img = b"wtns" + struct.pack("<II", 2, 2) + struct.pack("<IQI", 1, 40, 32) + R.to_bytes(32, "little") + struct.pack("<I", len(w))
    return img + struct.pack("<IQ", 2, 32 * len(w)) + b"".join(x.to_bytes(32, "little") for x in w)


def test_cli_prove_check_g2_parses_the_witness_first(tmp_path):
    k = GF.KnownLog(5, 1, 4)
    z, w = tmp_path / "c.zkey", tmp_path / "w.wtns"
    z.write_bytes(k.zkey)
    img = _wtns([1, 2, 3, 4, 5])
    outs = (tmp_path / "proof.json", tmp_path / "public.json")
    for flags in (("--check-g2",), ("--check-g2", "--check-g2")):
        p = _cli("groth16-prove", *flags, z, w, *outs[:1])
        assert p.returncode == 2 and "usage" in p.stderr and "--check-g2" in p.stderr, p
    w.write_bytes(img[:-1])
    for args in (("--check-g2", z, w) + outs, (z, w, "--check-g2") + outs):
        p = _cli("groth16-prove", *args)
        assert p.returncode == 2 and "wtns: truncated section 2" in p.stderr, p
    w.write_bytes(_wtns([1, 2, 3, 4]))
    p = _cli("groth16-prove", "--check-g2", z, w, *outs)
    assert p.returncode == 2 and "the witness has 4 elements, the zkey nVars = 5" in p.stderr, p
    assert not outs[0].exists() and not outs[1].exists()
