"""The Lagrange sections of a `.ptau` where there is no GPU: the identity that ptau_check_lagrange rests on, in plain integers (it
pins the definition that test_gpu_ptau_prepare.py uses, section 12's truncated last level included, and passes whatever the
library does), and what ptau_prepare_phase2, ptau_check_lagrange and the groth16-setup CLI refuse before they touch the device:
a malformed file, a file without prepared sections, a domain too large for the file, a workspace too small, usage errors."""
import os
import random
import struct
import subprocess
import sys

import pytest

import cwc_import
from tests import groth16_fixtures as GF
from tests import ptau_fixtures as PF

PKG = cwc_import.load()
R = GF.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETUP = os.path.join(ROOT, "circom-witnesscalc_amd", "groth16-setup")
CONTRIBUTE = os.path.join(ROOT, "circom-witnesscalc_amd", "groth16-contribute")
TAU, ALPHA, BETA = (random.Random(700).randrange(2, R) for _ in range(3))


# -- the identity -----------------------------------------------------------------------------------------------------------------
def levels_of(t, top):
    """[Lag_m of the first 2^m values of t] for m = 0 .. top; past the end of t the input is 0 (the point at infinity)"""
    padded = t + [0] * ((1 << top) - len(t))
    return [[t[0] % R]] + [PF.lag(m, padded[:1 << m]) for m in range(1, top + 1)]


@pytest.mark.parametrize("power", range(5))
def test_the_identity_in_plain_integers(power):
    """sum_m sum_k rho_{m,k} Lag_m[k] = sum_i c_i t_i mod r with c = sum_m Lag_m(rho_m), for the sections' scalars: the powers of
    tau up to level power (sections 13 to 15, times alpha or beta) and up to level power + 1 of (t_0 .. t_{2n-2}, 0) (section 12),
    over all levels and over each level alone; c_{2n-1} multiplies the missing input and is dropped"""
    rnd = random.Random(710 + power)
    n = 1 << power
    for scale, top in ((1, power + 1), (1, power), (ALPHA, power), (BETA, power)):
        t = [scale * pow(TAU, i, R) % R for i in range(2 * n - 1 if top == power + 1 else n)]
        lagrange = levels_of(t, top)
        if top == power + 1:
            assert lagrange[top] == PF.lag(top, t + [0])
        for m in range(top + 1 if top == power else power + 1):  # below section 12's last level: the Lagrange scalars of tau
            assert lagrange[m] == PF.lagrange_scalars(m, TAU, scale)
        rho = [[rnd.randrange(1 << 128) for _ in range(1 << m)] for m in range(top + 1)]
        for checked in [list(range(top + 1))] + [[m] for m in range(top + 1)]:
            left = sum(rho[m][k] * lagrange[m][k] for m in checked for k in range(1 << m)) % R
            c = [0] * (1 << top)
            for m in checked:
                for i, x in enumerate(levels_of(rho[m], m)[m]):
                    c[i] = (c[i] + x) % R
            assert left == sum(ci * ti for ci, ti in zip(c, t)) % R  # zip drops c_{2n-1} where t is one short


# -- refusals made before the device is touched -------------------------------------------------------------------------------------
def refused(call, *args, **kw):
    with pytest.raises(PKG.WitnessCalcError) as e:
        call(*args, **kw)
    return str(e.value)


def honest(power, prepared=False):
    return PF.write_ptau(power, TAU, ALPHA, BETA, prepared=prepared)


def test_malformed_files_are_refused_by_the_loader():
    data = honest(1)
    secs = PF.sections(1, TAU, ALPHA, BETA)
    for call in (PKG.ptau_prepare_phase2, PKG.ptau_check_lagrange):
        assert refused(call, b"") == "ptau: bad magic (not a .ptau file)"
        assert refused(call, b"zkey" + data[4:]) == "ptau: bad magic (not a .ptau file)"
        assert "unsupported version 2" in refused(call, PF.assemble(secs, version=2))
        assert "truncated section" in refused(call, data[:-1])
        assert "trailing bytes" in refused(call, data + b"\0")
        assert "missing section 4" in refused(call, PF.assemble(secs, order=[1, 2, 3, 5, 6, 7]))
        assert "duplicate section 3" in refused(call, PF.assemble(secs, order=[1, 2, 3, 3, 4, 5, 6, 7]))
        short = dict(secs)
        short[2] = secs[2][:-64]
        assert "section 2 (tauG1) has 128 bytes, 192 expected" in refused(call, PF.assemble(short))
        moved = dict(secs)
        moved[2] = secs[2][64:128] + secs[2][64:]
        assert "point 0 is not the G1 generator" in refused(call, PF.assemble(moved))
    assert "power 29 is above 28" in refused(PKG.ptau_prepare_phase2, PF.assemble({**secs, 1: PF.header(29)}))


def test_check_refuses_unprepared_files_and_large_domains():
    assert "no prepared sections 12 to 15" in refused(PKG.ptau_check_lagrange, honest(2))
    assert "no prepared sections 12 to 15" in refused(PKG.ptau_check_lagrange, honest(2), 1)
    partly = PF.sections(2, TAU, ALPHA, BETA, prepared=True)
    del partly[14]
    assert "no prepared sections 12 to 15" in refused(PKG.ptau_check_lagrange, PF.assemble(partly))
    for prepared in (False, True):  # the domain rule comes before the sections', as in the setup
        msg = refused(PKG.ptau_check_lagrange, honest(2, prepared), 2)
        assert "the circuit's domain 2^2 needs a ceremony of power 3 or more, this file has power 2" in msg
    with pytest.raises(PKG.WitnessCalcError, match="seed: 32 bytes expected"):
        PKG.ptau_check_lagrange(honest(2, True), 1, seed=b"short")


def test_check_names_point_faults_before_the_device():
    """a Lagrange point off its curve in a level that is read, then a monomial one: ptau_check's wording, found on the host"""
    secs = PF.sections(2, TAU, ALPHA, BETA, prepared=True)
    off = GF.lem(1) + GF.lem(3)
    bad = dict(secs)
    bad[14] = secs[14][:64 * 2] + off + secs[14][64 * 3:]
    assert refused(PKG.ptau_check_lagrange, PF.assemble(bad), 1) == "ptau: section 14 (lagrange alphaTauG1) point 2 is not on the G1 curve"
    assert refused(PKG.ptau_check_lagrange, PF.assemble(bad)) == "ptau: section 14 (lagrange alphaTauG1) point 2 is not on the G1 curve"
    bad = dict(secs)
    bad[2] = secs[2][:64] + off + secs[2][128:]
    assert refused(PKG.ptau_check_lagrange, PF.assemble(bad), 1) == "ptau: section 2 (tauG1) point 1 is not on the G1 curve"


def hollow_file(power):
    """a header of `power` and sections of the right sizes that hold the two generators and nothing else: enough for the loader"""
    n = 1 << power
    secs = {1: PF.header(power), 2: PF.python_points(1, [1]) + bytes(64 * (2 * n - 2)), 3: PF.python_points(2, [1]) + bytes(128 * (n - 1)),
            4: bytes(64 * n), 5: bytes(64 * n), 6: bytes(128), 7: struct.pack("<I", 0)}
    return PF.assemble(secs)


def test_a_workspace_too_small_is_refused_before_the_device(tmp_path):
    """CWC_GROTH16_WORKSPACE_MB = 1 against power 12, whose section 12 needs (2^14 - 1) 128 bytes on the device; a child process,
    so that the knob is the child's alone, through Python and through the CLI"""
    path = tmp_path / "hollow.ptau"
    path.write_bytes(hollow_file(12))
    env = dict(os.environ, CWC_GROTH16_WORKSPACE_MB="1")
    want = "(%d of them for all levels of one section), above the 1048576 of CWC_GROTH16_WORKSPACE_MB" % ((2 ** 14 - 1) * 128)
    code = ("import sys; sys.path.insert(0, %r); import cwc_import; P = cwc_import.load()\n"
            "try:\n    P.ptau_prepare_phase2(open(%r, 'rb').read())\nexcept P.WitnessCalcError as e:\n    print(e)\n" % (ROOT, str(path)))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and want in p.stdout and "ptau prepare: power 12 needs " in p.stdout, p
    p = subprocess.run([SETUP, "--prepare-ptau", str(path), str(tmp_path / "out.ptau")], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 2 and want in p.stderr and not (tmp_path / "out.ptau").exists(), p


def test_cli_usage_and_file_errors(tmp_path):
    ptau = tmp_path / "pot.ptau"
    ptau.write_bytes(honest(2))
    (tmp_path / "bad.ptau").write_bytes(honest(2)[:-1])
    path = lambda name: str(tmp_path / name)  # noqa: E731
    run = lambda *args: subprocess.run(list(args), capture_output=True, text=True, timeout=120)  # noqa: E731
    for args in (["--prepare-ptau"], ["--prepare-ptau", path("pot.ptau")], ["--prepare-ptau", path("pot.ptau"), path("o.ptau"), path("x")],
                 ["--check-lagrange"], ["--check-lagrange", "--domain-power", "1"], ["--check-lagrange", "--domain-power", "x", path("pot.ptau")],
                 ["--check-lagrange", "--domain-power", "29", path("pot.ptau")], ["--check-lagrange", path("pot.ptau"), path("x")],
                 ["--check-lagrange", "--lagrange", path("pot.ptau")]):
        p = run(SETUP, *args)
        assert p.returncode == 2 and "usage" in p.stderr and "--prepare-ptau" in p.stderr and "--check-lagrange" in p.stderr, (args, p)
    assert not (tmp_path / "o.ptau").exists()
    for args, frag in ((["--prepare-ptau", path("none.ptau"), path("o.ptau")], "cannot read"), (["--check-lagrange", path("none.ptau")], "cannot read"),
                       (["--prepare-ptau", path("bad.ptau"), path("o.ptau")], "truncated section"), (["--check-lagrange", path("bad.ptau")], "truncated section"),
                       (["--check-lagrange", path("pot.ptau")], "no prepared sections"),
                       (["--check-lagrange", "--domain-power", "2", path("pot.ptau")], "needs a ceremony of power 3 or more")):
        p = run(SETUP, *args)
        assert p.returncode == 2 and frag in p.stderr and p.stdout == "", (args, p)
    assert not (tmp_path / "o.ptau").exists()
    p = run(CONTRIBUTE, "--verify", "--check-lagrange", path("pot.ptau"))
    assert p.returncode == 2 and "usage: groth16-contribute" in p.stderr and "[--check-lagrange]" in p.stderr, p
