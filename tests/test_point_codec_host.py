"""The point codec of r1cs/point_codec_gfx950.hpp without a device: the model of tests/point_codec_cases.py against itself (anchors,
round trips, both root routes), the header's constants, and the case lists that tests/test_gpu_point_codec.py runs on an MI355X
through the host build of the header, tests/native/point_codec_host.cc, a stand-alone program under -fsanitize=address,undefined
that shares its per-record function with the device harness.  The device harness and r1cs/codec.hip are cross-compiled for gfx950;
every kernel of codec.hip must report ScratchSize 0."""
import os
import random
import re
import subprocess

import pytest

from tests import bn254_pairing as BP
from tests import groth16_fixtures as GF
from tests import point_codec_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R1CS = os.path.join(ROOT, "circom-witnesscalc_amd", "r1cs")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
Q = PC.Q


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("point_codec_host") / "point_codec_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + R1CS,
                           "-o", exe, os.path.join(ROOT, "tests", "native", "point_codec_host.cc")])
    return exe


def test_header_constants():
    """(q + 1) / 4, (q - 1) / 2 and the Montgomery form of 1/2, as the header's limbs spell them"""
    PC.check_header_constants()


def test_model_roots_by_two_routes():
    """the model's complex-method root against the norm route of tests/bn254_pairing.py, and the identity of the header's route on
    the inputs where its cases part: a1 = 0, a0 = 0, 0, +-1, squares and non-squares"""
    rnd = random.Random(5)
    F2 = PC.F2
    inputs = [(0, 0), (1, 0), (Q - 1, 0), (0, 1), (0, Q - 1), (4, 0), (Q - 4, 0)]
    inputs += [(rnd.randrange(Q), 0) for _ in range(20)] + [(0, rnd.randrange(Q)) for _ in range(20)]
    inputs += [(rnd.randrange(Q), rnd.randrange(Q)) for _ in range(60)]
    inputs += [F2.mul(x, x) for x in ((rnd.randrange(Q), rnd.randrange(Q)) for _ in range(60))]
    seen = set()
    for a in inputs:
        r1, r2 = PC.fq2_sqrt(a), BP.fq2_sqrt(a)
        if a[1] == 0 and r2 is None:   # that helper finds no pure-imaginary root (it never meets one on the twist)
            assert r1 is not None and r1[0] == 0
            r2 = r1
        assert (r1 is None) == (r2 is None), a
        branch = PC.kernel_branch(a)
        assert (branch == "none") == (r1 is None), a
        seen.add(branch)
        if r1 is not None:
            assert F2.mul(r1, r1) == a and r1 in (r2, F2.neg(r2))
            # the header's route, on integers
            s = PC.fq_sqrt((a[0] * a[0] + a[1] * a[1]) % Q)
            t = ((a[0] + s) % Q or (a[0] - s) % Q) * pow(2, -1, Q) % Q
            c = pow(t, PC.SQRT_EXP, Q)
            d = a[1] * pow(2 * c, Q - 2, Q) % Q
            root = (c, d) if c * c % Q == t else (d, c)
            assert c * c % Q in (t, -t % Q) and F2.mul(root, root) == a, a
    assert seen == {"none", "zero", "plus", "minus"}


def test_model_round_trips_and_refusals():
    for group, comp, dec in ((1, PC.g1_compress, PC.g1_decompress), (2, PC.g2_compress, PC.g2_decompress)):
        for p in PC.sample_points(group, 16):
            assert dec(comp(p)) == (PC.VALID, p)
        assert len(PC.refused_encodings(group, random.Random(1))) >= 9
    p = BP.twist_point_outside_subgroup(random.Random(4))   # the codec does not look at the subgroup
    assert PC.g2_decompress(PC.g2_compress(p)) == (PC.VALID, p)


@pytest.mark.parametrize("name", list(PC.FAMILIES))
def test_family_on_the_host(host_program, tmp_path, name):
    """every record of the family gives what the model says, no sanitizer report, the guard records untouched"""
    sections = PC.family(name)
    fin, fout = tmp_path / (name + ".in"), tmp_path / (name + ".out")
    PC.write_sections(fin, sections)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([host_program, str(fin), str(fout)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.strip() == "point_codec_host: %d sections" % len(sections)
    PC.check_outputs(fout, sections)


def test_device_harness_compiles_for_gfx950(tmp_path):
    """compile only (no GPU here): the harness of tests/test_gpu_point_codec.py must not arrive uncompilable"""
    assert os.path.exists(PC.build_device_harness(tmp_path, HIPCC))


def test_every_codec_kernel_without_scratch(tmp_path):
    """hipcc -Rpass-analysis=kernel-resource-usage on r1cs/codec.hip: each of its kernels reports ScratchSize 0"""
    p = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(R1CS, "codec.hip"), "-o", str(tmp_path / "c.o")], capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stderr)]
    assert len(scratch) == len(names), (names, scratch)
    for k in ("compress_points_kernel", "decompress_points_kernel", "compress_proofs_kernel", "decompress_proofs_kernel", "merge_status_kernel"):
        assert any(k in n for n in names), (k, names)
    assert sum("compress_points_kernel" in n for n in names) == 4   # compress and decompress, G1 and G2
    assert len(names) == 7 and all(s == 0 for s in scratch), list(zip(names, scratch))
