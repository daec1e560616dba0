"""The batched point multiplication out[i] = s_i P_i of the powers-of-tau ceremony on an MI355X (r1cs/ceremony.hip, through
bn254_g1_mul_batch_device and bn254_g2_mul_batch_device): both groups, both methods (signed windows with the table in LDS, and
double-and-add per thread), both forms, point by point against the plain-Python curve and against each other.  The points are
multiples of the generator with known logs, so the oracle is a fixed-base product and stays in seconds."""
import functools
import random

import numpy as np
import pytest

import cwc_import
from tests import ceremony_fixtures as CE
from tests import contribution_fixtures as CF
from tests import groth16_fixtures as GF

PKG = cwc_import.load()
R = GF.R
pytestmark = pytest.mark.gpu
METHODS, FORMS = ("window", "plain"), ("canonical", "montgomery")
WIDTH = 3  # the window of both groups in r1cs/ceremony.hip: the digit patterns below are written for it


def encode(group, form, p):
    if form == "canonical":
        return (CF.canonical_g1 if group == 1 else CF.canonical_g2)(p)
    return (GF.g1_bytes if group == 1 else GF.g2_bytes)(p)


def scalar_array(scalars):
    return np.frombuffer(b"".join(s.to_bytes(32, "little") for s in scalars), dtype=np.uint8).reshape(len(scalars), 32)


@functools.lru_cache(maxsize=None)
def bases(group, n, seed):
    """n logs (0: the point at infinity) and their affine points, made once"""
    rnd = random.Random(seed)
    logs = [rnd.randrange(1, R) for _ in range(n)]
    if n > 2:
        logs[1] = 0  # a point at infinity beside ordinary ones, and one at the end of the launch
        logs[-1] = 0
    curve = GF.G1 if group == 1 else GF.G2
    return tuple(logs), tuple(curve.gen_muls(logs))


def check(group, logs, points, scalars):
    """every method and form on the device against the Python curve: [s_i P_i] point by point"""
    import torch
    curve = GF.G1 if group == 1 else GF.G2
    n, width = len(logs), 64 * group
    want = curve.gen_muls([a * s % R for a, s in zip(logs, scalars)])
    assert any(w is None for w in want) or n < 3
    d_scalars = torch.from_numpy(scalar_array(scalars).copy()).cuda()
    got = {}
    for form in FORMS:
        pts = np.frombuffer(b"".join(encode(group, form, p) for p in points), dtype=np.uint8).reshape(n, width)
        d_points = torch.from_numpy(pts.copy()).cuda()
        expect = b"".join(encode(group, form, p) for p in want)
        for method in METHODS:
            call = PKG.bn254_g1_mul_batch_device if group == 1 else PKG.bn254_g2_mul_batch_device
            out = call(d_points, d_scalars, form=form, method=method)
            torch.cuda.synchronize()
            got[form, method] = out.cpu().numpy().tobytes()
            for i in range(n):
                assert got[form, method][i * width:(i + 1) * width] == expect[i * width:(i + 1) * width], (form, method, i, hex(scalars[i]))
        assert got[form, "window"] == got[form, "plain"]


@pytest.mark.parametrize("group,n", [(1, 1), (1, 63), (1, 64), (1, 65), (1, 257), (2, 1), (2, 63), (2, 64), (2, 65)])
def test_every_product_at_the_wave_and_workgroup_seams(group, n):
    logs, points = bases(group, n, 40 + group)
    rnd = random.Random(1000 * group + n)
    scalars = [rnd.randrange(R) for _ in range(n)]
    scalars[0] = R - 1
    if n > 3:
        scalars[2], scalars[3] = 0, 1
    check(group, logs, points, scalars)


def g2_edge_scalars():
    out = [0, 1, R - 1, (R - 1) // 2]
    for k in (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 191, 192, 250, 251, 252, 253):
        out += [1 << k, (1 << k) - 1]
    return out + CE.edge_scalars()[-8:]  # the digit patterns


@pytest.mark.parametrize("group", [1, 2])
def test_the_edge_scalars(group):
    """0, 1, r - 1, (r - 1) / 2, 2^k, 2^k - 1 and the digit patterns (every k in G1, a spread of them in G2)"""
    scalars = CE.edge_scalars() if group == 1 else g2_edge_scalars()
    assert group == 1 or len(scalars) <= 70
    logs, points = bases(group, len(scalars), 50 + group)
    check(group, logs, points, scalars)


@pytest.mark.parametrize("group", [1, 2])
def test_adjacent_lanes_with_different_signs_and_leading_zero_windows(group):
    """one wave: lane i has i leading zero windows, and its digits alternate in sign against its neighbour's; a lane with every
    digit -4 below the top, one with every digit 3, and one with zero digits between two nonzero ones"""
    n_win = CE.windows(WIDTH)
    scalars = []
    for lane in range(61):
        digits = [(1 + (lane + j) % 4) * (-1 if (lane + j) % 2 else 1) for j in range(n_win - 1 - lane)] + [1]
        scalars.append(sum(d << (WIDTH * j) for j, d in enumerate(digits)))
        assert CE.recode(scalars[-1], WIDTH) == digits + [0] * lane
    scalars.append(sum(-4 << (WIDTH * j) for j in range(n_win - 1)) + (2 << (WIDTH * (n_win - 1))))
    scalars.append(sum(3 << (WIDTH * j) for j in range(n_win - 1)))
    scalars.append((3 << (WIDTH * 70)) - 2)
    assert len(scalars) == 64 and all(0 < s < R for s in scalars)
    assert CE.recode(scalars[61], WIDTH) == [-4] * (n_win - 1) + [2] and CE.recode(scalars[63], WIDTH) == [-2] + [0] * 69 + [3] + [0] * 14
    logs, points = bases(group, 64, 60 + group)
    check(group, logs, points, scalars)


def test_the_aids_arguments():
    import torch
    pts, sc = torch.zeros((3, 64), dtype=torch.uint8, device="cuda"), torch.zeros((3, 32), dtype=torch.uint8, device="cuda")
    assert not PKG.bn254_g1_mul_batch_device(pts, sc).cpu().numpy().any()  # infinity stays infinity
    assert tuple(PKG.bn254_g2_mul_batch_device(torch.zeros((0, 128), dtype=torch.uint8, device="cuda"), sc[:0]).shape) == (0, 128)
    with pytest.raises(PKG.WitnessCalcError, match="form must be canonical or montgomery"):
        PKG.bn254_g1_mul_batch_device(pts, sc, form="jacobian")
    with pytest.raises(PKG.WitnessCalcError, match="method must be one of window, plain"):
        PKG.bn254_g1_mul_batch_device(pts, sc, method="bucket")
