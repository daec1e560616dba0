"""A `.ptau` writer for tests (iden3 binfile "ptau" v1, the layout in r1cs/ptau.cc) from known logs (tau, alpha, beta), on the
plain-Python curve of groth16_fixtures: the monomial sections 1 to 7 and, with prepared=True, the Lagrange sections 12 to 15 of
`powersoftau prepare phase2` (from Lagrange scalars, section 12 with its extra level).  sections() returns the bodies by id so
that a test can break one of them before assemble() joins them."""
import struct

from tests import groth16_fixtures as GF
from tests import qap_reference as QR

R, Q = GF.R, GF.Q


def python_points(group, scalars):
    """[k] -> the concatenated stored form (affine, Montgomery little-endian) of k G, on the Python curve"""
    if group == 1:
        return b"".join(map(GF.g1_bytes, GF.G1.gen_muls(scalars)))
    return b"".join(map(GF.g2_bytes, GF.G2.gen_muls(scalars)))


def lagrange_scalars(m, tau, c=1):
    """[c L_k(tau)] for the domain of 2^m points: Lag_m of the scalars c tau^i"""
    if m == 0:
        return [c % R]
    n = 1 << m
    w = QR.roots(m)[0]
    zf = (pow(tau, n, R) - 1) * pow(n, -1, R) % R
    xs, pref, x, acc = [], [], 1, 1
    for _ in range(n):  # the denominators tau - w^k with one inversion (Montgomery's trick)
        xs.append(x)
        pref.append(acc)
        acc = acc * (tau - x) % R
        x = x * w % R
    inv, out, f = pow(acc, -1, R), [0] * n, c * zf % R
    for k in range(n - 1, -1, -1):
        out[k] = f * xs[k] % R * (inv * pref[k] % R) % R
        inv = inv * (tau - xs[k]) % R
    return out


def lag(m, s):
    """Lag_m of any scalar sequence: [(1 / N) sum_i w_N^(-k i) s_i] (radix-2 recursion on plain integers)"""
    n = 1 << m
    assert len(s) == n and m >= 1

    def rec(x, w):  # [sum_i w^(k i) x_i]
        if len(x) == 1:
            return list(x)
        w2 = w * w % R
        ev, od = rec(x[0::2], w2), rec(x[1::2], w2)
        half, out, t = len(ev), [0] * len(x), 1
        for k in range(half):
            y = t * od[k] % R
            out[k], out[k + half] = (ev[k] + y) % R, (ev[k] - y) % R
            t = t * w % R
        return out

    ni = pow(n, -1, R)
    return [ni * x % R for x in rec([x % R for x in s], pow(QR.roots(m)[0], -1, R))]


def header(power, ceremony_power=None, n8=32, q=Q):
    return struct.pack("<I", n8) + q.to_bytes(32, "little") + struct.pack("<II", power, power if ceremony_power is None else ceremony_power)


def sections(power, tau, alpha, beta, prepared=False, lagrange_tau=None, ceremony_power=None, n_contributions=0, points=python_points):
    """{id: body}.  lagrange_tau: the tau the prepared sections are written from (default: tau itself)."""
    n = 1 << power
    t = [pow(tau, i, R) for i in range(2 * n - 1)]
    secs = {1: header(power, ceremony_power),
            2: points(1, t),
            3: points(2, t[:n]),
            4: points(1, [alpha * x % R for x in t[:n]]),
            5: points(1, [beta * x % R for x in t[:n]]),
            6: points(2, [beta]),
            7: struct.pack("<I", n_contributions)}
    if prepared:
        lt = tau if lagrange_tau is None else lagrange_tau
        levels = lambda c, top: [x for m in range(top + 1) for x in lagrange_scalars(m, lt, c)]  # noqa: E731
        secs[12] = points(1, levels(1, power + 1))
        secs[13] = points(2, levels(1, power))
        secs[14] = points(1, levels(alpha, power))
        secs[15] = points(1, levels(beta, power))
    return secs


def assemble(secs, order=None, extra=(), magic=b"ptau", version=1):
    """order: section ids as they follow each other in the file (an id may repeat); extra: (id, body) pairs appended"""
    ids = list(order) if order is not None else sorted(secs)
    body = b"".join(GF.section(i, secs[i]) for i in ids) + b"".join(GF.section(i, b) for i, b in extra)
    return magic + struct.pack("<II", version, len(ids) + len(extra)) + body


def write_ptau(power, tau, alpha, beta, **kw):
    return assemble(sections(power, tau, alpha, beta, **kw))
