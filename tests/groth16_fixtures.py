"""Plain-Python BN254 for the Groth16 prover's tests: Fq, Fq2 = Fq[u]/(u^2 + 1), G1 and G2 in affine and Jacobian form,
fixed-base windowed tables (thousands of k G in seconds), a `.zkey` writer (snarkjs's Groth16 layout, include/
graph_witness_groth16.h), a trapdoor zkey over the planted systems of r1cs_fixtures (every proof has known discrete logs), and
a known-log zkey of arithmetic progressions for large sizes."""
import struct

from tests import qap_reference as QR
from tests import r1cs_fixtures as F

R = F.R
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
MONT = (1 << 256) % Q

# -- fields -------------------------------------------------------------------------------------------------------------------


class Fq1:
    zero, one = 0, 1

    @staticmethod
    def add(a, b):
        return (a + b) % Q

    @staticmethod
    def sub(a, b):
        return (a - b) % Q

    @staticmethod
    def mul(a, b):
        return a * b % Q

    @staticmethod
    def inv(a):
        return pow(a, Q - 2, Q)

    @staticmethod
    def neg(a):
        return -a % Q


class Fq2:
    zero, one = (0, 0), (1, 0)

    @staticmethod
    def add(a, b):
        return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)

    @staticmethod
    def sub(a, b):
        return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)

    @staticmethod
    def mul(a, b):
        return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)

    @staticmethod
    def inv(a):
        n = pow((a[0] * a[0] + a[1] * a[1]) % Q, Q - 2, Q)
        return (a[0] * n % Q, -a[1] * n % Q)

    @staticmethod
    def neg(a):
        return (-a[0] % Q, -a[1] % Q)


B1 = 3
B2 = Fq2.mul((3, 0), Fq2.inv((9, 1)))  # 3 / (9 + u), the twist constant
G1_GEN = (1, 2)
G2_GEN = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
           11559732032986387107991004021392285783925812861821192530917403151452391805634),
          (8495653923123431417604973247489272438418190587263600148770280649306958101930,
           4082367875863433681332203403145435568316851327593401208105741076214120093531))


# -- curves: affine points are (x, y) or None (infinity); Jacobian (X, Y, Z) with Z = 0 for infinity ---------------------------
class Curve:
    def __init__(self, f, b, gen):
        self.f, self.b, self.gen = f, b, gen
        self.inf = (f.one, f.one, f.zero)
        self._table = None

    def on_curve(self, p):
        if p is None:
            return True
        f = self.f
        x, y = p
        return f.mul(y, y) == f.add(f.mul(f.mul(x, x), x), self.b)

    def jac(self, p):
        return self.inf if p is None else (p[0], p[1], self.f.one)

    def is_inf(self, j):
        return j[2] == self.f.zero

    def dbl(self, j):
        f = self.f
        if self.is_inf(j):
            return j
        X, Y, Z = j
        A, Bq = f.mul(X, X), f.mul(Y, Y)
        C = f.mul(Bq, Bq)
        D = f.sub(f.mul(f.add(X, Bq), f.add(X, Bq)), f.add(A, C))
        D = f.add(D, D)
        E = f.add(f.add(A, A), A)
        X3 = f.sub(f.mul(E, E), f.add(D, D))
        C8 = f.add(C, C)
        C8 = f.add(C8, C8)
        C8 = f.add(C8, C8)
        Y3 = f.sub(f.mul(E, f.sub(D, X3)), C8)
        Z3 = f.mul(f.add(Y, Y), Z)
        return (X3, Y3, Z3)

    def add(self, p, q):
        f = self.f
        if self.is_inf(p):
            return q
        if self.is_inf(q):
            return p
        X1, Y1, Z1 = p
        X2, Y2, Z2 = q
        Z1Z1, Z2Z2 = f.mul(Z1, Z1), f.mul(Z2, Z2)
        U1, U2 = f.mul(X1, Z2Z2), f.mul(X2, Z1Z1)
        S1, S2 = f.mul(f.mul(Y1, Z2), Z2Z2), f.mul(f.mul(Y2, Z1), Z1Z1)
        if U1 == U2:
            return self.dbl(p) if S1 == S2 else self.inf
        H, Rr = f.sub(U2, U1), f.sub(S2, S1)
        HH = f.mul(H, H)
        HHH = f.mul(H, HH)
        V = f.mul(U1, HH)
        X3 = f.sub(f.sub(f.mul(Rr, Rr), HHH), f.add(V, V))
        Y3 = f.sub(f.mul(Rr, f.sub(V, X3)), f.mul(S1, HHH))
        return (X3, Y3, f.mul(f.mul(Z1, Z2), H))

    def neg_aff(self, p):
        return None if p is None else (p[0], self.f.neg(p[1]))

    def to_affine(self, j):
        if self.is_inf(j):
            return None
        f = self.f
        zi = f.inv(j[2])
        zi2 = f.mul(zi, zi)
        return (f.mul(j[0], zi2), f.mul(j[1], f.mul(zi2, zi)))

    def batch_affine(self, js):
        """Jacobian list -> affine list with one inversion (Montgomery's trick)"""
        f = self.f
        zs = [j[2] for j in js if not self.is_inf(j)]
        pref, acc = [], f.one
        for z in zs:
            pref.append(acc)
            acc = f.mul(acc, z)
        inv = f.inv(acc) if zs else f.one
        invs = [None] * len(zs)
        for i in range(len(zs) - 1, -1, -1):
            invs[i] = f.mul(inv, pref[i])
            inv = f.mul(inv, zs[i])
        out, k = [], 0
        for j in js:
            if self.is_inf(j):
                out.append(None)
                continue
            zi = invs[k]
            k += 1
            zi2 = f.mul(zi, zi)
            out.append((f.mul(j[0], zi2), f.mul(j[1], f.mul(zi2, zi))))
        return out

    def mul(self, p, k):
        """k p by double-and-add (any point)"""
        acc, base = self.inf, self.jac(p)
        for bit in bin(k)[2:] if k > 0 else "":
            acc = self.dbl(acc)
            if bit == "1":
                acc = self.add(acc, base)
        return acc

    def table(self):
        """T[w][d] = d 2^(8 w) G (affine), w < 32, d < 256; built once"""
        if self._table is None:
            rows, base = [], self.jac(self.gen)
            for _ in range(32):
                row, acc = [self.inf], self.inf
                for _ in range(255):
                    acc = self.add(acc, base)
                    row.append(acc)
                rows.append(row)
                for _ in range(8):
                    base = self.dbl(base)
            flat = self.batch_affine([p for row in rows for p in row])
            self._table = [flat[256 * w:256 * w + 256] for w in range(32)]
        return self._table

    def gen_mul_jac(self, k):
        t = self.table()
        k %= R
        acc = self.inf
        for w in range(32):
            d = (k >> (8 * w)) & 255
            if d:
                acc = self.add(acc, self.jac(t[w][d]))
        return acc

    def gen_muls(self, ks):
        """[k G] (affine or None) for many k, fixed-base"""
        return self.batch_affine([self.gen_mul_jac(k) for k in ks])


G1 = Curve(Fq1, B1, G1_GEN)
G2 = Curve(Fq2, B2, G2_GEN)


# -- encodings ----------------------------------------------------------------------------------------------------------------
def lem(x):
    """Fq element -> 32-byte Montgomery little-endian (snarkjs LEM)"""
    return (x * MONT % Q).to_bytes(32, "little")


def g1_bytes(p):
    return bytes(64) if p is None else lem(p[0]) + lem(p[1])


def g2_bytes(p):
    return bytes(128) if p is None else lem(p[0][0]) + lem(p[0][1]) + lem(p[1][0]) + lem(p[1][1])


def proof_bytes(a, b, c):
    """affine pi_A (G1), pi_B (G2), pi_C (G1) -> the library's 256 canonical bytes"""
    out = b""
    for p, words in ((a, 2), (b, 4), (c, 2)):
        if p is None:
            out += bytes(32 * words)
        elif words == 2:
            out += p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")
        else:
            out += b"".join(x.to_bytes(32, "little") for x in (p[0][0], p[0][1], p[1][0], p[1][1]))
    return out


def section(sid, body):
    return struct.pack("<IQ", sid, len(body)) + body


def write_zkey(n_vars, n_public, domain_size, alpha1, beta1, beta2, gamma2, delta1, delta2, ic, a, b1, b2, c, h, coefs=(),
               protocol=1, order=None, q=Q, r=R, n8q=32, n8r=32, version=1, extra=()):
    """points affine (None = infinity) -> .zkey bytes; coefs: (matrix, constraint, signal, value) tuples"""
    hdr = struct.pack("<I", n8q) + q.to_bytes(n8q, "little") + struct.pack("<I", n8r) + r.to_bytes(n8r, "little")
    hdr += struct.pack("<III", n_vars, n_public, domain_size)
    hdr += g1_bytes(alpha1) + g1_bytes(beta1) + g2_bytes(beta2) + g2_bytes(gamma2) + g1_bytes(delta1) + g2_bytes(delta2)
    s4 = struct.pack("<I", len(coefs)) + b"".join(struct.pack("<III", m, k, s) + (v * MONT % R).to_bytes(32, "little")
                                                   for m, k, s, v in coefs)
    secs = {1: struct.pack("<I", protocol), 2: hdr, 3: b"".join(map(g1_bytes, ic)), 4: s4, 5: b"".join(map(g1_bytes, a)),
            6: b"".join(map(g1_bytes, b1)), 7: b"".join(map(g2_bytes, b2)), 8: b"".join(map(g1_bytes, c)),
            9: b"".join(map(g1_bytes, h)), 10: b""}
    ids = list(order) if order else sorted(secs)
    body = b"".join(section(i, secs[i]) for i in ids) + b"".join(extra)
    return b"zkey" + struct.pack("<II", version, len(ids) + len(extra)) + body


# -- trapdoor zkey ------------------------------------------------------------------------------------------------------------
class Trapdoor:
    """A zkey with known tau, alpha, beta, gamma, delta for a constraint system (r1cs_fixtures combinations); proof logs known."""

    def __init__(self, constraints, n_wires, n_pub, tau=None, alpha=None, beta=None, gamma=None, delta=None, seed=1, tweak=None):
        import random
        rnd = random.Random(seed)
        self.cons, self.n_wires, self.n_pub = constraints, n_wires, n_pub
        pick = lambda v: v if v is not None else rnd.randrange(2, R)  # noqa: E731
        self.tau, self.alpha, self.beta, self.gamma, self.delta = map(pick, (tau, alpha, beta, gamma, delta))
        n_c = len(constraints)
        _, p = QR.domain(n_c, n_pub)
        n = self.n = 1 << p
        wn, g = QR.roots(p)
        tau = self.tau
        # n-domain Lagrange basis at tau: L_k = (tau^n - 1) / n * w^k / (tau - w^k)
        zf = (pow(tau, n, R) - 1) * pow(n, -1, R) % R
        pw = [pow(wn, k, R) for k in range(n)]
        lag = [zf * pw[k] * pow(tau - pw[k], -1, R) % R for k in range(n)]
        u, v, w = [0] * n_wires, [0] * n_wires, [0] * n_wires
        for k, (ca, cb, cc) in enumerate(constraints):
            for wire, co in F.terms(ca):
                u[wire] = (u[wire] + co * lag[k]) % R
            for wire, co in F.terms(cb):
                v[wire] = (v[wire] + co * lag[k]) % R
            for wire, co in F.terms(cc):
                w[wire] = (w[wire] + co * lag[k]) % R
        for s in range(n_pub + 1):
            u[s] = (u[s] + lag[n_c + s]) % R
        self.u, self.v, self.w = u, v, w
        # 2n-domain basis at the odd points g w^j: (tau^2n - 1) / 2n * x / (tau - x)
        zf2 = (pow(tau, 2 * n, R) - 1) * pow(2 * n, -1, R) % R
        self.lh = [zf2 * (g * pw[j]) * pow(tau - g * pw[j], -1, R) % R for j in range(n)]
        di, gi = pow(self.delta, -1, R), pow(self.gamma, -1, R)
        al, be = self.alpha, self.beta
        self.k_ic = [(be * u[i] + al * v[i] + w[i]) * gi % R for i in range(n_pub + 1)]
        self.k_c = [(be * u[i] + al * v[i] + w[i]) * di % R for i in range(n_pub + 1, n_wires)]
        self.k_h = [x * di % R for x in self.lh]
        logs = {"a": list(u), "b1": list(v), "b2": list(v), "c": list(self.k_c), "h": list(self.k_h), "ic": list(self.k_ic)}
        if tweak:
            tweak(logs)
        self.logs = logs
        p1 = G1.gen_muls(logs["a"] + logs["b1"] + logs["c"] + logs["h"] + logs["ic"] + [al, be, self.delta])
        nv, nc_, nh = n_wires, len(logs["c"]), n
        a_pts, p1 = p1[:nv], p1[nv:]
        b1_pts, p1 = p1[:nv], p1[nv:]
        c_pts, p1 = p1[:nc_], p1[nc_:]
        h_pts, p1 = p1[:nh], p1[nh:]
        ic_pts, p1 = p1[:n_pub + 1], p1[n_pub + 1:]
        alpha1, beta1, delta1 = p1
        p2 = G2.gen_muls(logs["b2"] + [be, self.gamma, self.delta])
        b2_pts, (beta2, gamma2, delta2) = p2[:nv], p2[nv:]
        self.zkey = write_zkey(n_wires, n_pub, n, alpha1, beta1, beta2, gamma2, delta1, delta2, ic_pts, a_pts, b1_pts, b2_pts,
                               c_pts, h_pts)

    def proof_logs(self, w, r, s, h=None):
        """(a, b, c) discrete logs of the proof of row w (ints, reduced mod r here) with randomness r, s"""
        w = [x % R for x in w]
        if h is None:
            h = QR.h_of(self.cons, self.n_pub, w)
        L = self.logs
        a = (self.alpha + sum(x * y for x, y in zip(w, L["a"])) + r * self.delta) % R
        b = (self.beta + sum(x * y for x, y in zip(w, L["b2"])) + s * self.delta) % R
        b1 = (self.beta + sum(x * y for x, y in zip(w, L["b1"])) + s * self.delta) % R
        c = (sum(x * y for x, y in zip(w[self.n_pub + 1:], L["c"])) + sum(x * y for x, y in zip(h, L["h"])) + s * a + r * b1
             - r * s * self.delta) % R
        return a, b, c

    def verifies(self, w, a, b, c):
        """Groth16's verification equation in the exponent: a b == alpha beta + gamma ic + delta c (mod r)"""
        ic = sum(x % R * y for x, y in zip(w[:self.n_pub + 1], self.k_ic)) % R
        return a * b % R == (self.alpha * self.beta + self.gamma * ic + self.delta * c) % R

    def want_bytes(self, logs):
        """[(a, b, c)] -> uint8 [B, 256] of a G1, b G2, c G1"""
        import numpy as np
        p1 = G1.gen_muls([x for a, _, c in logs for x in (a, c)])
        p2 = G2.gen_muls([b for _, b, _ in logs])
        out = b"".join(proof_bytes(p1[2 * i], p2[i], p1[2 * i + 1]) for i in range(len(logs)))
        return np.frombuffer(out, dtype=np.uint8).reshape(len(logs), 256).copy()


# -- known-log zkey (arithmetic progressions) ---------------------------------------------------------------------------------
def progression(curve, k0, d, n):
    """n affine points P_i = (k0 + i d) G, one affine addition each; -> (points, logs)"""
    f = curve.f
    p0, dd = curve.to_affine(curve.gen_mul_jac(k0)), curve.to_affine(curve.gen_mul_jac(d))
    out, logs, p = [], [], p0
    for i in range(n):
        out.append(p)
        logs.append((k0 + i * d) % R)
        if p is None:
            p = dd
        elif p[0] == dd[0]:
            p = curve.to_affine(curve.add(curve.jac(p), curve.jac(dd)))
        else:
            lam = f.mul(f.sub(dd[1], p[1]), f.inv(f.sub(dd[0], p[0])))
            x3 = f.sub(f.sub(f.mul(lam, lam), p[0]), dd[0])
            p = (x3, f.sub(f.mul(lam, f.sub(p[0], x3)), p[1]))
    return out, logs


class KnownLog:
    """A zkey of arithmetic progressions (not a valid setup): every MSM's discrete log is a dot product."""

    def __init__(self, n_vars, n_public, domain_size, seed=3):
        import random
        rnd = random.Random(seed)
        self.n_vars, self.n_pub, self.n = n_vars, n_public, domain_size
        self.alpha, self.beta, self.delta, self.gamma = (rnd.randrange(1, R) for _ in range(4))
        a, self.la = progression(G1, rnd.randrange(R), rnd.randrange(R), n_vars)
        b1, self.lb1 = progression(G1, rnd.randrange(R), rnd.randrange(R), n_vars)
        b2, self.lb2 = progression(G2, rnd.randrange(R), rnd.randrange(R), n_vars)
        c, self.lc = progression(G1, rnd.randrange(R), rnd.randrange(R), n_vars - n_public - 1)
        h, self.lh = progression(G1, rnd.randrange(R), rnd.randrange(R), domain_size)
        ic = [None] * (n_public + 1)
        g1 = G1.gen_muls([self.alpha, self.beta, self.delta])
        g2 = G2.gen_muls([self.beta, self.gamma, self.delta])
        self.zkey = write_zkey(n_vars, n_public, domain_size, g1[0], g1[1], g2[0], g2[1], g1[2], g2[2], ic, a, b1, b2, c, h)

    def proof_logs(self, w, h, r, s):
        w = [x % R for x in w]
        a = (self.alpha + sum(x * y for x, y in zip(w, self.la)) + r * self.delta) % R
        b = (self.beta + sum(x * y for x, y in zip(w, self.lb2)) + s * self.delta) % R
        b1 = (self.beta + sum(x * y for x, y in zip(w, self.lb1)) + s * self.delta) % R
        c = (sum(x * y for x, y in zip(w[self.n_pub + 1:], self.lc)) + sum(x * y for x, y in zip(h, self.lh)) + s * a + r * b1
             - r * s * self.delta) % R
        return a, b, c
