"""The pairing tower of r1cs/fq12_gfx950.hpp without a device: the case lists of tests/fq12_tower_cases.py (the same ones
tests/test_gpu_fq12_tower.py runs on an MI355X) through the host build of the header, tests/native/fq12_tower_host.cc, a
stand-alone program under -fsanitize=address,undefined that shares its per-record function with the device harness.  This proves
the oracle, the class lists and every expected value on the CPU; the device harness is cross-compiled for gfx950 as a compile
check."""
import os
import random
import subprocess

import pytest

from tests import bn254_pairing as BP
from tests import fq12_tower_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R1CS = os.path.join(ROOT, "circom-witnesscalc_amd", "r1cs")
Q = TC.Q


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fq12_tower_host") / "fq12_tower_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + R1CS,
                           "-o", exe, os.path.join(ROOT, "tests", "native", "fq12_tower_host.cc")])
    return exe


def test_the_oracles_additions():
    """what tests/fq12_tower_cases.py adds to the flat oracle, against the oracle's own power and mul"""
    rnd = random.Random(7)
    a = tuple(rnd.randrange(Q) for _ in range(12))
    assert TC.conj12(a) == BP.power(a, Q ** 6)
    assert TC.flat(TC.tower(a)) == a
    x = (rnd.randrange(Q), rnd.randrange(Q))
    assert TC.flat(TC.F2.mul(x, TC.XI)) == BP.mul(TC.flat(x), BP.mul(BP.W3, BP.W3))   # xi = w^6
    assert TC.flat([0, 0, 1, 0]) == BP.W2 and BP.mul(BP.mul(BP.W2, BP.W2), BP.W2) == TC.flat(TC.XI)   # v = w^2, v^3 = xi
    l = [(rnd.randrange(Q), rnd.randrange(Q)) for _ in range(3)]
    assert TC.tower(TC.line_flat(*l)) == [l[0][0], l[0][1], 0, 0, 0, 0, l[1][0], l[1][1], l[2][0], l[2][1], 0, 0]   # c0.b0, c1.b0, c1.b1
    e = BP.power(a, TC.EASY_EXP)
    assert BP.power(e, TC.HARD_EXP) == BP.final_exp(a)


@pytest.mark.parametrize("name", list(TC.FAMILIES))
def test_family_on_the_host(host_program, tmp_path, name):
    """every record of the family gives the oracle's value, every coefficient reduced, no sanitizer report"""
    sections = TC.family(name)
    assert [op for op, _ in sections] == TC.FAMILIES[name]
    fin, fout = tmp_path / (name + ".in"), tmp_path / (name + ".out")
    TC.write_sections(fin, sections)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([host_program, str(fin), str(fout)], capture_output=True, text=True, env=env, timeout=1800)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.strip() == "fq12_tower_host: %d sections" % len(sections)
    TC.check_outputs(fout, sections)


def test_device_harness_compiles_for_gfx950(tmp_path):
    """compile only (no GPU here): the harness of tests/test_gpu_fq12_tower.py must not arrive uncompilable"""
    exes = TC.build_device_harness(tmp_path, os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    assert sorted(exes) == sorted(TC.FAMILIES) and all(os.path.exists(e) for e in exes.values())
