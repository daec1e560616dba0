"""Folded KZG openings (include/graph_witness_kzg.h) on plain integers: the specification that r1cs/kzg.hip's fold kernels and
kzg.cc's open_fold and verify_fold are written against, with no constant taken from the library.

A group is K polynomials of one length, a point z and a challenge gamma.  f = sum_k gamma^k p_k (gamma^0 = 1 also for gamma = 0);
open_fold gives y_k = p_k(z) and the quotient of f at z; with a known tau the commitments and the witness are multiples of G1
whose logs are the polynomials' values at tau, and the check e(C_f - y_f G1 + z W, G2) = e(W, tau G2) is an identity of logs."""
from tests.kzg_model import R, horner


def fold(polys, gamma):
    """the coefficients of sum_k gamma^k p_k, by Horner in gamma from the last polynomial down"""
    gamma %= R
    acc = [0] * len(polys[0])
    for p in reversed(polys):
        assert len(p) == len(acc)
        acc = [(c + gamma * a) % R for c, a in zip(p, acc)]
    return acc


def fold_values(values, gamma):
    """sum_k gamma^k v_k"""
    acc = 0
    for v in reversed(values):
        acc = (v + gamma * acc) % R
    return acc


def open_fold(polys, z, gamma):
    """(ys, q): y_k = p_k(z), and the quotient of the folded polynomial at z"""
    z %= R
    ys = [horner([c % R for c in p], z)[0] for p in polys]
    return ys, horner(fold(polys, gamma), z)[1]


def logs(polys, z, gamma, tau):
    """(the logs of C_0 .. C_{K-1}, ys, the log of W) of the honest folded opening over the SRS of tau"""
    ys, q = open_fold(polys, z, gamma)
    return [horner([c % R for c in p], tau)[0] for p in polys], ys, horner(q, tau)[0]


def check(c_logs, z, gamma, ys, w_log, tau):
    """the folded check in logs: C_f - y_f + z w = tau w"""
    c_f, y_f = fold_values(c_logs, gamma % R), fold_values(ys, gamma % R)
    return (c_f - y_f + z * w_log - tau * w_log) % R == 0
