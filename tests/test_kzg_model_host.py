"""The tiled evaluate-and-quotient recursion of tests/kzg_model.py against direct Horner and synchronous division on Python
integers, at the seams of the run, the wave, the tile and the second level.  The model is the specification of r1cs/kzg.hip and
takes no constant from the library, so this file passes with or without it; tests/test_gpu_kzg_quotient.py holds the kernels to
the same oracle.  Small tiles (a wave of 4, runs of 1 and 2) keep the second and third level cheap."""
import random

import pytest

from tests import kzg_model as M

R = M.R
SHAPES = [(8, 1, 4), (16, 2, 4), (16, 4, 4), (256, 1, 64), (1024, 4, 64)]  # (tile, run, wave)


def seams(tile, run, wave):
    ns = {1, 2, wave - 1, wave, wave + 1, tile - 1, tile, tile + 1, 2 * tile + 1, 3 * tile + 1, run, run + 1, wave * run - 1, wave * run + 1}
    if run > 1:
        ns.add(run - 1)
    if tile <= 16:
        ns |= {tile * tile - 1, tile * tile, tile * tile + 1, tile ** 3 + 1}
    return sorted(n for n in ns if n >= 1)


@pytest.mark.parametrize("tile,run,wave", SHAPES)
def test_the_recursion_is_horner_and_division(tile, run, wave):
    rnd = random.Random(tile * 31 + run)
    for n in seams(tile, run, wave):
        c = [rnd.randrange(R) for _ in range(n)]
        for z in (0, 1, R - 1, rnd.randrange(R)):
            assert M.eval_quotient(c, z, tile, run, wave) == M.horner(c, z), (n, z)


def test_the_levels():
    assert [M.levels(n, 256) for n in (1, 256, 257, 65536, 65537)] == [1, 1, 2, 2, 3]
    assert M.levels(4097, 16) == 4 and M.levels(0, 8) == 1


@pytest.mark.parametrize("tile,run,wave", SHAPES[:3])
def test_edge_coefficients_and_roots(tile, run, wave):
    rnd = random.Random(5)
    n = tile * tile + 1
    for c in ([0] * n, [R - 1] * n, [7] + [0] * (n - 1), [0] * (n - 1) + [9], [R + 3, 2 * R + 1] + [rnd.randrange(R) for _ in range(n - 2)]):
        z = rnd.randrange(R)
        assert M.eval_quotient(c, z, tile, run, wave) == M.horner([x % R for x in c], z)
    # a root: p = (X - a) g has p(a) = 0 and the quotient g
    a, g = rnd.randrange(R), [rnd.randrange(R) for _ in range(n - 1)]
    p = [(-a * g[0]) % R] + [(g[i - 1] - a * g[i]) % R for i in range(1, n - 1)] + [g[-1]]
    assert M.eval_quotient(p, a, tile, run, wave) == (0, g)


def test_the_definition():
    """s_i = sum_{j >= i} c_j z^(j-i), spelled out"""
    rnd = random.Random(9)
    c, z = [rnd.randrange(R) for _ in range(11)], rnd.randrange(R)
    s = [sum(c[j] * pow(z, j - i, R) for j in range(i, len(c))) % R for i in range(len(c))]
    assert M.horner(c, z) == (s[0], s[1:])
    assert M.horner([], z) == (0, []) and M.eval_quotient([], z, 8, 1, 4) == (0, [])
    assert M.eval_quotient([5], z, 8, 1, 4) == (5, [])
