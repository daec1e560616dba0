"""The evaluate-and-quotient kernels of the KZG layer (r1cs/kzg.hip) on an MI355X through their aid, for every tile size the
library instantiates, against synchronous division on Python integers (tests/kzg_model.horner): y and every q_i byte for byte.

The lengths are the seams of the kernel, computed from the tile: around a wave (63, 64, 65), around a thread's run and a wave of
runs for the tiles with runs longer than one, around one tile, two and three tiles and a bit, and for the smallest tile around
tile^2, where the recursion takes its second level (65 537 coefficients are three launches of totals and three of apply).  Every
length runs as one launch of 11 different (polynomial, point) pairs, so a mix-up of the pair index shows: every kind of
coefficients with a random point, and random coefficients with every kind of point.

Wall time on an MI355X: under 0.1 s per case below three tiles, about 1.5 s for the three cases around 256^2 (the Python oracle)."""
import random

import numpy as np
import pytest

import cwc_import
from tests import kzg_model as M

PKG = cwc_import.load()
R = M.R
TILES = PKG.kzg_tiles()

pytestmark = pytest.mark.gpu


def lengths(tile):
    run = tile // 256
    ns = {1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1}
    if tile == TILES[0]:
        ns |= {tile * tile - 1, tile * tile, tile * tile + 1}
    else:
        ns |= {run - 1, run, run + 1, 64 * run - 1, 64 * run + 1, 3 * tile + 1}
    return sorted(n for n in ns if n >= 1)


CASES = [(t, n) for t in TILES for n in lengths(t)]


def with_root(rnd, n):
    """(p, a): p = (X - a) g for a random g of n - 1 coefficients (n = 1: the zero polynomial)"""
    a = rnd.randrange(R)
    if n == 1:
        return [0], a
    g = [rnd.randrange(R) for _ in range(n - 1)]
    return [(-a * g[0]) % R] + [(g[i - 1] - a * g[i]) % R for i in range(1, n - 1)] + [g[-1]], a


def pairs(n, seed):
    """[(coefficients as stored, any value below 2^256; point)]"""
    rnd = random.Random(seed)
    rand = lambda: [rnd.randrange(R) for _ in range(n)]  # noqa: E731
    big = rand()
    for i, v in zip(rnd.sample(range(n), min(n, 4)), (R, R + 5, (1 << 256) - 1, 5 * R + 1)):
        big[i] = v
    out = [(rand(), rnd.randrange(R)), ([0] * n, rnd.randrange(R)), ([R - 1] * n, rnd.randrange(R)), ([rnd.randrange(1, R)] + [0] * (n - 1), rnd.randrange(R)),
           ([0] * (n - 1) + [rnd.randrange(1, R)], rnd.randrange(R)), (big, rnd.randrange(R)),
           (rand(), 0), (rand(), 1), (rand(), R - 1), ([R - 1] * n, R - 1)]
    out.append(with_root(rnd, n))
    return out


def le(values):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), dtype=np.uint8)


@pytest.mark.parametrize("tile,n", CASES)
def test_y_and_q_are_python_s(tile, n):
    import torch
    ps = pairs(n, tile * 1000003 + n)
    k = len(ps)
    d_polys = torch.from_numpy(np.stack([le(c) for c, _ in ps]).reshape(k, n, 32).copy()).cuda()
    d_zs = torch.from_numpy(le([z for _, z in ps]).reshape(k, 32).copy()).cuda()
    d_ys, d_qs = PKG.kzg_eval_quotient_device(d_polys, d_zs, tile=tile)
    torch.cuda.synchronize()
    ys, qs = d_ys.cpu().numpy(), d_qs.cpu().numpy()
    assert ys.shape == (k, 32) and qs.shape == (k, n - 1, 32)
    for i, (c, z) in enumerate(ps):
        want_y, want_q = M.horner([x % R for x in c], z)
        assert bytes(ys[i]) == want_y.to_bytes(32, "little"), (tile, n, i)
        assert np.array_equal(qs[i].reshape(-1), le(want_q)), (tile, n, i)
    assert int.from_bytes(bytes(ys[-1]), "little") == 0  # the point of the last pair is a root


def test_the_default_tile_is_the_last_and_a_point_above_r_is_reduced():
    import torch
    rnd = random.Random(77)
    n = TILES[-1] + 3
    c = [rnd.randrange(R) for _ in range(n)]
    z = R + 12345
    d_polys = torch.from_numpy(le(c).reshape(1, n, 32).copy()).cuda()
    d_zs = torch.from_numpy(le([z]).reshape(1, 32).copy()).cuda()
    got = [PKG.kzg_eval_quotient_device(d_polys, d_zs, tile=t) for t in (None, TILES[-1], TILES[0])]
    torch.cuda.synchronize()
    want_y, want_q = M.horner(c, z % R)
    for d_ys, d_qs in got:
        assert bytes(d_ys.cpu().numpy()[0]) == want_y.to_bytes(32, "little")
        assert np.array_equal(d_qs.cpu().numpy().reshape(-1), le(want_q))


def test_more_pairs_than_one_launch_takes():
    """The pair index is the grid's second dimension, so a batch goes out 32 768 pairs at a time: the pairs past that seam get
    their own polynomial and point."""
    import torch
    rnd = random.Random(78)
    k, n = 32768 + 5, 3
    cs = [[rnd.randrange(R) for _ in range(n)] for _ in range(k)]
    zs = [rnd.randrange(R) for _ in range(k)]
    d_polys = torch.from_numpy(le([x for c in cs for x in c]).reshape(k, n, 32).copy()).cuda()
    d_zs = torch.from_numpy(le(zs).reshape(k, 32).copy()).cuda()
    d_ys, d_qs = PKG.kzg_eval_quotient_device(d_polys, d_zs, tile=TILES[0])
    torch.cuda.synchronize()
    want = [M.horner(c, z) for c, z in zip(cs, zs)]
    assert np.array_equal(d_ys.cpu().numpy().reshape(-1), le([y for y, _ in want]))
    assert np.array_equal(d_qs.cpu().numpy().reshape(-1), le([x for _, q in want for x in q]))


def test_an_unknown_tile_and_empty_inputs():
    import torch
    d_polys = torch.zeros((2, 5, 32), dtype=torch.uint8).cuda()
    d_zs = torch.zeros((2, 32), dtype=torch.uint8).cuda()
    with pytest.raises(PKG.WitnessCalcError, match=r"tile 512 is not instantiated"):
        PKG.kzg_eval_quotient_device(d_polys, d_zs, tile=512)
    d_ys, d_qs = PKG.kzg_eval_quotient_device(d_polys[:, :0], d_zs)
    torch.cuda.synchronize()
    assert d_qs.shape == (2, 0, 32) and not d_ys.cpu().numpy().any()
    d_ys, d_qs = PKG.kzg_eval_quotient_device(d_polys[:0], d_zs[:0])
    assert d_ys.shape == (0, 32) and d_qs.shape == (0, 4, 32)
