"""Plain-Python restatement of the Groth16 witness map (include/graph_witness_r1cs.h, gwb_r1cs_qap_*), independent of the
C++ library and its kernels.  The roots are derived from r itself.

- qap_rows: the QAP rows a, b, c of one witness row (constraint rows in file order, then the input rows, then zeros);
- h_direct: h by the definition, O(n^2): interpolate on the domain, evaluate at the coset points g w^j;
- h_ntt: h by a recursive radix-2 NTT, O(n log n), a second and independent route;
- h_at: h_j at chosen j by Lagrange evaluation on the domain, O(n) per point, for domains too large for the other two.
"""
from tests.r1cs_fixtures import R, terms

MAX_POWER = 27


def two_adicity():
    s, q = 0, R - 1
    while q % 2 == 0:
        q //= 2
        s += 1
    return s


def smallest_nonresidue():
    z = 2
    while pow(z, (R - 1) // 2, R) != R - 1:  # Euler's criterion
        z += 1
    return z


S = two_adicity()
W_MAX = pow(smallest_nonresidue(), (R - 1) >> S, R)  # a primitive 2^S-th root of unity


def domain(n_constraints, n_pub):
    """(N, p): N = nC + nPub + 1 rows, p >= 1 the smallest with 2^p >= N (may exceed MAX_POWER: the library refuses it)"""
    n_rows = n_constraints + n_pub + 1
    p = 1
    while (1 << p) < n_rows:
        p += 1
    return n_rows, p


def roots(p):
    """(w_n, g) for n = 2^p: w_n = w_28^(2^(28-p)), g = w_28^(2^(27-p))"""
    assert 1 <= p <= MAX_POWER
    return pow(W_MAX, 1 << (S - p), R), pow(W_MAX, 1 << (S - 1 - p), R)


def _dot(lc, w):
    return sum(c * w[i] for i, c in terms(lc)) % R


def qap_rows(constraints, n_pub, w):
    """w: a witness row (ints, reduced mod r here) -> (a, b, c), each of length n"""
    w = [x % R for x in w]
    _, p = domain(len(constraints), n_pub)
    n = 1 << p
    a = [_dot(con[0], w) for con in constraints] + [w[s] for s in range(n_pub + 1)]
    b = [_dot(con[1], w) for con in constraints] + [0] * (n_pub + 1)
    a += [0] * (n - len(a))
    b += [0] * (n - len(b))
    return a, b, [x * y % R for x, y in zip(a, b)]


def _dft_direct(v, root):
    n = len(v)
    out = []
    for k in range(n):
        step, x, acc = pow(root, k, R), 1, 0
        for i in range(n):
            acc += v[i] * x
            x = x * step % R
        out.append(acc % R)
    return out


def h_direct(a, b, c):
    """h_j = A(g w^j) B(g w^j) - C(g w^j) with A the interpolant of a on the domain; O(n^2)"""
    n = len(a)
    p = n.bit_length() - 1
    wn, g = roots(p)
    n_inv, w_inv = pow(n, -1, R), pow(wn, -1, R)
    vals = []
    for v in (a, b, c):
        coef = [x * n_inv % R for x in _dft_direct(v, w_inv)]  # A(X) = sum coef_i X^i
        pts = [g * pow(wn, j, R) % R for j in range(n)]
        evals = []
        for x in pts:
            acc, xp = 0, 1
            for ci in coef:
                acc += ci * xp
                xp = xp * x % R
            evals.append(acc % R)
        vals.append(evals)
    return [(x * y - z) % R for x, y, z in zip(*vals)]


def ntt(v, root):
    """sum_i v_i root^(i k) for k < len(v), recursive radix 2"""
    n = len(v)
    if n == 1:
        return [v[0] % R]
    even, odd = ntt(v[0::2], root * root % R), ntt(v[1::2], root * root % R)
    out, t = [0] * n, 1
    for k in range(n // 2):
        x = odd[k] * t % R
        out[k], out[k + n // 2] = (even[k] + x) % R, (even[k] - x) % R
        t = t * root % R
    return out


def h_ntt(a, b, c):
    """h by inverse NTT, coset scaling, forward NTT; O(n log n)"""
    n = len(a)
    p = n.bit_length() - 1
    wn, g = roots(p)
    n_inv, w_inv = pow(n, -1, R), pow(wn, -1, R)
    vals = []
    for v in (a, b, c):
        coef = ntt(v, w_inv)
        gi, scaled = n_inv, []
        for x in coef:
            scaled.append(x * gi % R)
            gi = gi * g % R
        vals.append(ntt(scaled, wn))
    return [(x * y - z) % R for x, y, z in zip(*vals)]


def h_at(a, b, c, js):
    """h_j for j in js by Lagrange evaluation: A(x) = (x^n - 1) / n * sum_i a_i w^i / (x - w^i), and x^n = g^n = -1"""
    n = len(a)
    p = n.bit_length() - 1
    wn, g = roots(p)
    factor = (R - 2) * pow(n, -1, R) % R  # (x^n - 1) / n
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * wn % R
    out = []
    for j in js:
        x = g * pw[j] % R
        sa = sb = sc = 0
        for i in range(n):
            if a[i] or b[i] or c[i]:
                t = pw[i] * pow(x - pw[i], -1, R)
                sa += a[i] * t
                sb += b[i] * t
                sc += c[i] * t
        A, B, C = (factor * s % R for s in (sa, sb, sc))
        out.append((A * B - C) % R)
    return out


def h_of(constraints, n_pub, w):
    """h of one witness row, by h_ntt"""
    return h_ntt(*qap_rows(constraints, n_pub, w))


def h_bytes(h):
    """list of ints -> uint8 [n, 32] canonical little-endian"""
    import numpy as np
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in h), dtype=np.uint8).reshape(len(h), 32).copy()
