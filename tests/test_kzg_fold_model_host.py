"""The plain-integer specification of the folded KZG openings (tests/kzg_fold_model.py) against the single-polynomial one
(tests/kzg_model.py): folding commutes with the quotient and with evaluation, and the folded check is an identity in the logs over
a known tau.  Random groups, with gamma in {0, 1, r - 1} and z = tau among them.  No GPU and no library."""
import random

import pytest

from tests import kzg_fold_model as FM
from tests import kzg_model as M

R = M.R
TAU = random.Random(77).randrange(2, R)


def groups():
    rnd = random.Random(2025)
    out = []
    for k, n in ((1, 1), (1, 9), (2, 2), (3, 17), (4, 5), (17, 33)):
        for gamma in (0, 1, R - 1, rnd.randrange(R)):
            for z in (0, TAU, R - 1, rnd.randrange(R)):
                out.append(([[rnd.randrange(R) for _ in range(n)] for _ in range(k)], z, gamma))
    return out


GROUPS = groups()


def test_gamma_to_the_zero_is_one_also_for_gamma_zero():
    polys = [[3, 4], [5, 6], [7, 8]]
    assert FM.fold(polys, 0) == [3, 4] and FM.fold(polys, 1) == [15, 18] and FM.fold(polys, 2) == [3 + 10 + 28, 4 + 12 + 32]
    assert FM.fold(polys, R + 2) == FM.fold(polys, 2) and FM.fold_values([3, 5, 7], 0) == 3


def test_the_folded_quotient_is_the_fold_of_the_quotients():
    for polys, z, gamma in GROUPS:
        _, q = FM.open_fold(polys, z, gamma)
        each = [M.horner(p, z)[1] for p in polys]
        assert q == (FM.fold(each, gamma) if each[0] else [])


def test_the_folded_value_is_the_fold_of_the_values():
    for polys, z, gamma in GROUPS:
        ys, _ = FM.open_fold(polys, z, gamma)
        assert ys == [M.horner(p, z)[0] for p in polys]
        assert M.horner(FM.fold(polys, gamma), z)[0] == FM.fold_values(ys, gamma)


def test_the_check_identity_holds_in_logs():
    for polys, z, gamma in GROUPS:
        cs, ys, w = FM.logs(polys, z, gamma, TAU)
        assert FM.check(cs, z, gamma, ys, w, TAU)
        if len(polys[0]) > 1:
            wrong = list(ys)
            wrong[-1] = (wrong[-1] + 1) % R
            assert FM.check(cs, z, gamma, wrong, w, TAU) == (len(polys) > 1 and gamma == 0)  # gamma = 0 binds y_0 alone


@pytest.mark.parametrize("gamma", (0, 1, R - 1, 12345))
def test_one_polynomial_is_the_plain_opening_for_any_gamma(gamma):
    rnd = random.Random(gamma % 1000)
    p, z = [rnd.randrange(R) for _ in range(12)], rnd.randrange(R)
    ys, q = FM.open_fold([p], z, gamma)
    assert ([ys[0]], q) == ([M.horner(p, z)[0]], M.horner(p, z)[1])
