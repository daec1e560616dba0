"""The Groth16 witness map's definition (include/graph_witness_r1cs.h, gwb_r1cs_qap_*) restated in plain Python
(tests/qap_reference.py): the roots derived from r, two independent routes to h that must agree, the divisibility property
every h has, the domain sizes at their edges, and the witness-h CLI's usage errors.  CPU only."""
import os
import random
import subprocess

import pytest

import cwc_import
from tests import qap_reference as Q
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
R = F.R
CLI = os.path.join(os.path.dirname(PKG.R1CS_LIB_PATH), "witness-h")


def _random_system(rnd, n_wires, n_constraints, n_pub):
    def lc():
        return {rnd.randrange(n_wires): rnd.choice([1, R - 1, rnd.randrange(R)]) for _ in range(rnd.randrange(0, 4))}
    cons = [(lc(), lc(), lc()) for _ in range(n_constraints)]
    w = [1] + [rnd.randrange(R) for _ in range(n_wires - 1)]
    assert n_pub < n_wires
    return cons, w


def test_root_of_unity_from_r():
    assert Q.two_adicity() == 28
    assert Q.smallest_nonresidue() == 5
    assert pow(Q.W_MAX, 1 << 28, R) == 1
    assert pow(Q.W_MAX, 1 << 27, R) == R - 1  # order exactly 2^28
    # the root ffjavascript and arkworks use
    assert Q.W_MAX == 19103219067921713944291392827692070036145651957329286315305642004821462161904
    for p in (1, 5, 17, 27):
        wn, g = Q.roots(p)
        assert pow(wn, 1 << p, R) == 1 and pow(wn, 1 << (p - 1), R) == R - 1
        assert g * g % R == wn and pow(g, 1 << p, R) == R - 1  # g^n = -1: Z(g w^j) = -2


def test_direct_and_ntt_agree():
    rnd = random.Random(5)
    for p in list(range(1, 9)) + [10]:
        n = 1 << p
        a = [rnd.randrange(R) for _ in range(n)]
        b = [rnd.randrange(R) if rnd.random() < 0.8 else 0 for _ in range(n)]
        c = [x * y % R for x, y in zip(a, b)]
        assert Q.h_direct(a, b, c) == Q.h_ntt(a, b, c), p
    # and both against the Lagrange evaluation at a few points
    n = 1 << 6
    a, b = [rnd.randrange(R) for _ in range(n)], [rnd.randrange(R) for _ in range(n)]
    c = [x * y % R for x, y in zip(a, b)]
    h = Q.h_ntt(a, b, c)
    js = [0, 1, 17, n - 1]
    assert Q.h_at(a, b, c, js) == [h[j] for j in js]


def test_h_divisible_by_vanishing_polynomial():
    """c = a o b makes A B - C vanish on the domain, so A B - C = H Z with deg H <= n - 2: interpolating h_j / Z(g w^j) on the
    coset gives a polynomial whose coefficient n - 1 is zero.  Holds for any witness, satisfying or not, whatever the order."""
    rnd = random.Random(7)
    for n_c, n_pub in ((0, 0), (1, 0), (5, 2), (30, 3), (200, 10)):
        cons, w = _random_system(rnd, 40, n_c, n_pub)
        a, b, c = Q.qap_rows(cons, n_pub, w)
        h = Q.h_ntt(a, b, c)
        n = len(h)
        wn, g = Q.roots(n.bit_length() - 1)
        z_inv = pow(R - 2, -1, R)
        coef = Q.ntt([x * z_inv % R for x in h], pow(wn, -1, R))  # n * H(g X) coefficients
        assert coef[n - 1] == 0, (n_c, n_pub)
        assert any(coef) or not any(b), (n_c, n_pub)  # (not vacuous: H is not zero unless b is)
        # a wrong c (not a o b) breaks it
        c2 = list(c)
        c2[0] = (c2[0] + 1) % R
        coef2 = Q.ntt([x * z_inv % R for x in Q.h_ntt(a, b, c2)], pow(wn, -1, R))
        assert coef2[n - 1] != 0


def test_qap_rows_layout():
    cons = [({1: 2}, {2: 3}, {3: 1}), ({}, {}, {0: 1})]
    w = [1, 5, 7, 11, R + 4]  # an element above r is reduced
    a, b, c = Q.qap_rows(cons, 2, w)
    assert len(a) == 8  # N = 2 + 2 + 1 = 5 -> n = 8
    assert a == [10, 0, 1, 5, 7, 0, 0, 0]
    assert b == [21, 0, 0, 0, 0, 0, 0, 0]
    assert c == [210, 0, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("n_c,n_pub", [(0, 0), (1, 0), (0, 1), (2, 1), (3, 0), (6, 1), (7, 1), (1000, 23), (1001, 23), (4095, 0),
                                       (4090, 5), (4091, 5), (65535, 0), (65536, 0)])
def test_domain_edges(pkg, n_c, n_pub):
    """N = nC + nPub + 1 exactly a power of two, and one above it; the library's qap_info agrees with the restatement"""
    n_rows, p = Q.domain(n_c, n_pub)
    assert (1 << p) >= n_rows and (p == 1 or (1 << (p - 1)) < n_rows)
    n_wires = n_pub + 2
    cons = [({}, {}, {})] * n_c
    r = PKG.R1cs(F.write_r1cs(n_wires, cons, n_pub_out=n_pub // 2, n_pub_in=n_pub - n_pub // 2))
    info = r.qap_info()
    assert info == {"n_rows": n_rows, "domain_power": p, "domain_size": 1 << p, "workspace_bytes_per_row": 2 * 32 << p}


def test_domain_edge_values():
    assert Q.domain(0, 0) == (1, 1)
    assert Q.domain(1, 0) == (2, 1)
    assert Q.domain(2, 1) == (4, 2)
    assert Q.domain(3, 1) == (5, 3)
    assert Q.domain((1 << 27) - 1, 0) == (1 << 27, 27)
    assert Q.domain(1 << 27, 0) == ((1 << 27) + 1, 28)


def test_witness_h_cli_usage(tmp_path):
    assert os.path.exists(CLI), CLI
    r = subprocess.run([CLI], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    r = subprocess.run([CLI, str(tmp_path / "missing.r1cs"), str(tmp_path / "w.wtns"), str(tmp_path / "h.bin")], capture_output=True, text=True)
    assert r.returncode == 2 and "cannot read" in r.stderr
    bad = tmp_path / "bad.r1cs"
    bad.write_bytes(b"nope")
    wt = tmp_path / "w.wtns"
    wt.write_bytes(b"wtns")
    r = subprocess.run([CLI, str(bad), str(wt), str(tmp_path / "h.bin")], capture_output=True, text=True)
    assert r.returncode == 2 and "bad magic" in r.stderr
    good = tmp_path / "c.r1cs"
    good.write_bytes(F.write_r1cs(2, [({1: 1}, {1: 1}, {1: 1})]))
    r = subprocess.run([CLI, str(good), str(wt), str(tmp_path / "h.bin")], capture_output=True, text=True)
    assert r.returncode == 2 and "wtns: bad magic" in r.stderr
    assert not (tmp_path / "h.bin").exists()
