"""The Groth16 key setup's host side (include/graph_witness_groth16_setup.h): the trapdoor refusals of gwb_groth16_setup,
which are made before the device is touched and so hold on a machine without one, and the groth16-setup CLI's exit status 2
for usage, file and trapdoor-file errors."""
import os
import random
import subprocess

import pytest

import cwc_import
from tests import qap_reference as QR
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
R = F.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "circom-witnesscalc_amd", "groth16-setup")
NAMES = ("tau", "alpha", "beta", "gamma", "delta")
N_CONSTRAINTS, N_PUB = 11, 3  # 15 rows: the domain is 2^4


def _r1cs_bytes():
    rnd = random.Random(31)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(N_CONSTRAINTS)]
    pl = F.planted_system(rnd, 4, shapes, [1, R - 1, 2, None])
    return F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=2)


@pytest.fixture(scope="module")
def r1():
    r = PKG.R1cs(_r1cs_bytes())
    assert r.qap_info()["domain_power"] == 4
    return r


GOOD = (5, 7, 11, 13, 17)


def _with(i, v):
    t = list(GOOD)
    t[i] = v
    return tuple(t)


@pytest.mark.parametrize("i", range(5))
def test_zero_value_is_refused(r1, i):
    with pytest.raises(PKG.WitnessCalcError, match=r"%s is 0" % NAMES[i]):
        PKG.groth16_setup(r1, _with(i, 0))


@pytest.mark.parametrize("i", range(5))
def test_value_r_is_refused(r1, i):
    with pytest.raises(PKG.WitnessCalcError, match=r"%s is not below r" % NAMES[i]):
        PKG.groth16_setup(r1, _with(i, R))


def test_tau_on_either_domain_is_refused(r1):
    wn, g = QR.roots(4)
    assert pow(wn, 16, R) == 1 and pow(g, 16, R) == R - 1
    for tau in (R - 1, pow(wn, 3, R), g * wn % R):
        assert pow(tau, 32, R) == 1
        with pytest.raises(PKG.WitnessCalcError, match=r"tau satisfies tau\^\(2n\) = 1"):
            PKG.groth16_setup(r1, _with(0, tau))


def test_trapdoor_shape_is_refused(r1):
    with pytest.raises(PKG.WitnessCalcError, match="5 values"):
        PKG.groth16_setup(r1, (1, 2, 3, 4))
    with pytest.raises(PKG.WitnessCalcError, match="gamma"):
        PKG.groth16_setup(r1, _with(3, 1 << 256))


def _cli(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_cli_usage_and_file_errors(tmp_path):
    (tmp_path / "c.r1cs").write_bytes(_r1cs_bytes())
    c, z = tmp_path / "c.r1cs", tmp_path / "c.zkey"
    for args in ((), (c,), (c, z, tmp_path / "vk.json", "extra"), ("--trapdoor", c, z), (c, z, "--trapdoor")):
        p = _cli(*args)
        assert p.returncode == 2 and "usage" in p.stderr, (args, p)
    p = _cli(tmp_path / "missing.r1cs", z)
    assert p.returncode == 2 and "cannot read" in p.stderr
    (tmp_path / "bad.r1cs").write_bytes(b"r1cx" + bytes(20))
    p = _cli(tmp_path / "bad.r1cs", z)
    assert p.returncode == 2 and "bad magic" in p.stderr
    p = _cli("--trapdoor", tmp_path / "missing.txt", c, z)
    assert p.returncode == 2 and "cannot read" in p.stderr
    assert not z.exists()


@pytest.mark.parametrize("text, message", [
    ("5 7 11 13", "4 values, 5 expected"),
    ("5 7 0x0b 13 17", "beta is not a decimal integer"),
    ("5 7 11 -13 17", "gamma is not a decimal integer"),
    ("5 7 11 13 %d" % (1 << 256), "delta is not a decimal integer below 2\\^256"),
    ("5\n7\t11 13 %d\n" % R, "delta is not below r"),
    ("%d 7 11 13 17" % (R + 5), "tau is not below r"),
    ("5 0 11 13 17", "alpha is 0"),
    ("%d 7 11 13 17" % (R - 1), "tau satisfies"),
])
def test_cli_trapdoor_file_errors(tmp_path, text, message):
    import re
    (tmp_path / "c.r1cs").write_bytes(_r1cs_bytes())
    (tmp_path / "t.txt").write_text(text)
    p = _cli("--trapdoor", tmp_path / "t.txt", tmp_path / "c.r1cs", tmp_path / "c.zkey")
    assert p.returncode == 2, p
    assert re.search(message, p.stderr), p.stderr
    assert not (tmp_path / "c.zkey").exists()
