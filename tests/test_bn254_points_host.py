"""The stored form of BN254 points without a device: the host build of r1cs/bn254_points_gfx950.hpp (a stand-alone program under
-fsanitize=address,undefined, tests/native/bn254_points_host.cc) against the curve code of tests/groth16_fixtures.py, for both
groups and both forms.  The header is what the loaders check points with and what the kernels decode and encode them with."""
import os
import random
import subprocess

import pytest

from tests import groth16_fixtures as GF

Q = GF.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COORDINATE, CURVE, NONE = 0, 1, 3
MONT_INV = pow(GF.MONT, -1, Q)
GROUPS = {1: (GF.G1, 2), 2: (GF.G2, 4)}  # group -> curve, coordinate slots
CASES = [(g, form) for g in (1, 2) for form in "mc"]


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bn254_points_host") / "bn254_points_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "bn254_points_host.cc")])
    return exe


def run_host(exe, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.split("\n")[:-1]


def slots_of(group, p):
    """the coordinate values of an affine point in stored order; infinity is all zero"""
    n = GROUPS[group][1]
    if p is None:
        return [0] * n
    return [p[0], p[1]] if group == 1 else [p[0][0], p[0][1], p[1][0], p[1][1]]


def point_of(group, slots):
    return (slots[0], slots[1]) if group == 1 else ((slots[0], slots[1]), (slots[2], slots[3]))


def stored(form, slots, raw=()):
    """the stored bytes of the coordinate values; the slots named in `raw` hold their value as it is, in either form"""
    return b"".join(v.to_bytes(32, "little") if form == "c" or k in raw else GF.lem(v) for k, v in enumerate(slots))


def meaning(form, v):
    """the field element that the raw 32-byte value v below q stands for"""
    return v if form == "c" else v * MONT_INV % Q


def points(group):
    curve = GROUPS[group][0]
    rnd = random.Random(40 + group)
    return [curve.gen, curve.neg_aff(curve.gen)] + [curve.to_affine(curve.mul(curve.gen, rnd.randrange(2, 1 << 24))) for _ in range(3)]


def faults(exe, group, form, images):
    got = run_host(exe, ["F %d %s %s" % (group, form, b.hex()) for b in images])
    assert len(got) == len(images)
    return [int(l.split()[1]) for l in got]


@pytest.mark.parametrize("group,form", CASES)
def test_valid_points_and_infinity_round_trip(host_program, group, form):
    curve = GROUPS[group][0]
    pts = points(group) + [None]
    assert all(curve.on_curve(p) for p in pts)
    images = [stored(form, slots_of(group, p)) for p in pts]
    assert images[-1] == bytes(32 * GROUPS[group][1])
    assert faults(host_program, group, form, images) == [NONE] * len(pts)
    got = run_host(host_program, ["R %d %s %s" % (group, form, b.hex()) for b in images])
    assert got == ["R 1 " + b.hex() for b in images]


@pytest.mark.parametrize("group,form", CASES)
def test_q_in_a_slot_is_a_coordinate_fault_and_q_minus_1_a_curve_fault(host_program, group, form):
    curve, n = GROUPS[group]
    base = slots_of(group, points(group)[2])
    at_q, below_q, alone = [], [], []
    for k in range(n):
        at_q.append(stored(form, base[:k] + [Q] + base[k + 1:], raw=(k,)))
        below_q.append(stored(form, base[:k] + [Q - 1] + base[k + 1:], raw=(k,)))
        assert not curve.on_curve(point_of(group, base[:k] + [meaning(form, Q - 1)] + base[k + 1:]))
        alone.append(stored(form, [0] * k + [Q] + [0] * (n - k - 1), raw=(k,)))  # q reduces to 0: not to be taken for infinity
    assert faults(host_program, group, form, at_q) == [COORDINATE] * n
    assert faults(host_program, group, form, below_q) == [CURVE] * n
    assert faults(host_program, group, form, alone) == [COORDINATE] * n
    got = run_host(host_program, ["R %d %s %s" % (group, form, b.hex()) for b in at_q + below_q])
    assert [l.split()[1] for l in got] == ["0"] * n + ["1"] * n
    assert [l.split()[2] for l in got[n:]] == [b.hex() for b in below_q]  # an off-curve point is still decoded and encoded


@pytest.mark.parametrize("group,form", CASES)
def test_off_curve_points_and_the_order_of_the_two_faults(host_program, group, form):
    curve, n = GROUPS[group]
    off, both = [], []
    for p in points(group):
        s = slots_of(group, p)
        s[n - 1] = (s[n - 1] + 1) % Q  # y + 1, or y + u
        assert not curve.on_curve(point_of(group, s))
        off.append(stored(form, s))
        for k in range(n - 1):  # q, which reduces to 0, in another slot: still off the curve, and out of range
            t = s[:k] + [0] + s[k + 1:]
            assert not curve.on_curve(point_of(group, t))
            both.append(stored(form, s[:k] + [Q] + s[k + 1:], raw=(k,)))
    swapped = slots_of(group, points(group)[3])[::-1]
    assert not curve.on_curve(point_of(group, swapped))
    off.append(stored(form, swapped))
    assert faults(host_program, group, form, off) == [CURVE] * len(off)
    assert faults(host_program, group, form, both) == [COORDINATE] * len(both)


def test_curve_constants_and_generators(host_program):
    b, g = run_host(host_program, ["B", "G"])
    assert b == "B 1 1"  # curve_b<G1>() is Montgomery 3, curve_b<G2>() is 3 / (9 + u) by fq2_inv
    want1 = stored("c", slots_of(1, GF.G1_GEN)).hex()
    want2 = stored("c", slots_of(2, GF.G2_GEN)).hex()
    assert g == "G 1 1 1 %s %s" % (want1, want2)
    assert GF.G1.on_curve(GF.G1_GEN) and GF.G2.on_curve(GF.G2_GEN)
