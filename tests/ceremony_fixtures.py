"""Plain-Python powers-of-tau ceremony records for the tests: section 7 of a `.ptau` written and read, the challenges, the three
proofs of knowledge of a record, restated from include/graph_witness_groth16_ceremony.h with hashlib's BLAKE2b,
groth16_fixtures.Curve and contribution_fixtures.hash_to_g2; and a model of the signed-digit recoding of the device's windowed
multiplication (r1cs/ceremony.hip)."""
import struct

from tests import contribution_fixtures as CF
from tests import groth16_fixtures as GF

R, Q = GF.R, GF.Q
H, U1, U2 = CF.H, CF.U1, CF.U2
SECRETS = ("tau", "alpha", "beta")
# (name, is G2) in record order: the five after-values, then the nine key points
POINTS = (("tau_g1", False), ("tau_g2", True), ("alpha_g1", False), ("beta_g1", False), ("beta_g2", True), ("tau_g1_s", False), ("tau_g1_sx", False),
          ("alpha_g1_s", False), ("alpha_g1_sx", False), ("beta_g1_s", False), ("beta_g1_sx", False), ("tau_g2_spx", True), ("alpha_g2_spx", True),
          ("beta_g2_spx", True))
NO_RECORDS = struct.pack("<I", 0)
RECORD_FIXED = 3 * 64 + 2 * 128 + 6 * 64 + 3 * 128 + 216 + 64 + 8


# -- the recoding ---------------------------------------------------------------------------------------------------------------
def windows(w):
    return -(-254 // w)


def recode(s, w):
    """The signed digits of s for the width w, lowest window first, from the bottom with a carry: d = window + carry, and
    d >= 2^(w-1) gives d - 2^w and a carry.  The top window takes what is left of s, so that its carry would show."""
    n, half, digits, carry = windows(w), 1 << (w - 1), [], 0
    for j in range(n - 1):
        d = ((s >> (w * j)) & ((1 << w) - 1)) + carry
        carry = 1 if d >= half else 0
        digits.append(d - (carry << w))
    digits.append((s >> (w * (n - 1))) + carry)
    return digits


def recode_offset(s, w):
    """The same digits as the kernel takes them: window j of s + C minus 2^(w-1), C = sum_j 2^(w-1) 2^(w j); the top window is
    every bit of s + C from its lowest bit on."""
    n, half = windows(w), 1 << (w - 1)
    k = s + sum(half << (w * j) for j in range(n))
    assert k < 1 << 256
    return [((k >> (w * j)) & ((1 << w) - 1)) - half for j in range(n - 1)] + [(k >> (w * (n - 1))) - half]


def edge_scalars():
    """0, 1, r - 1, (r - 1) / 2, 2^k and 2^k - 1 for k < 254, and the digit patterns 88..8 and ff..f below r (44..4 and 77..7 in
    octal), among them 0x0ff..f, whose carry runs through every window"""
    out = [0, 1, R - 1, (R - 1) // 2]
    for k in range(254):
        out += [1 << k, (1 << k) - 1]
    out += [int(top + nibble * 63, 16) for nibble in "8f" for top in "012"]  # 0x0ff..f: the carry runs through every window
    out += [int(digit * 84, 8) for digit in "47"]  # the same for windows of three bits
    assert all(0 <= s < R for s in out)
    return out


# -- records --------------------------------------------------------------------------------------------------------------------
def key_transcript(challenge, j, g1_s, g1_sx):
    return H(challenge + bytes([j]) + U1(g1_s) + U1(g1_sx))


def key_point(challenge, j, g1_s, g1_sx):
    """g2_sp of secret j"""
    return CF.hash_to_g2(key_transcript(challenge, j, g1_s, g1_sx))


class Record:
    """pts: {name: affine point or None} for the fourteen names of POINTS"""

    def __init__(self, pts, next_challenge=bytes(64), type=0, params=b"", partial_hash=bytes(216)):
        self.pts, self.next_challenge, self.type, self.params, self.partial_hash = dict(pts), next_challenge, type, params, partial_hash

    def pub(self):
        return b"".join((U2 if g2 else U1)(self.pts[name]) for name, g2 in POINTS)

    def stored(self):
        return (b"".join((GF.g2_bytes if g2 else GF.g1_bytes)(self.pts[name]) for name, g2 in POINTS) + self.partial_hash + self.next_challenge
                + struct.pack("<II", self.type, len(self.params)) + self.params)

    def canonical(self):
        return {name: (CF.canonical_g2 if g2 else CF.canonical_g1)(self.pts[name]) for name, g2 in POINTS}


def anchors(tau, alpha, beta):
    """the five points a record continues, of a file written from the logs (tau, alpha, beta)"""
    g1 = lambda k: GF.G1.to_affine(GF.G1.gen_mul_jac(k))  # noqa: E731
    g2 = lambda k: GF.G2.to_affine(GF.G2.gen_mul_jac(k))  # noqa: E731
    return {"tau_g1": g1(tau), "tau_g2": g2(tau), "alpha_g1": g1(alpha), "beta_g1": g1(beta), "beta_g2": g2(beta)}


def first_challenge(section1):
    return H(section1)


def contribution(challenge, logs, secrets, nonces, name="", derive=key_point):
    """The record that a contribution with `secrets` = (tau', alpha', beta') and `nonces` appends to a file whose logs are
    `logs` = (tau, alpha, beta), after the challenge `challenge`; derive: the challenge point's derivation."""
    after = tuple(a * b % R for a, b in zip(logs, secrets))
    pts = anchors(*after)
    for j, nm in enumerate(SECRETS):
        g1_s = GF.G1.to_affine(GF.G1.gen_mul_jac(nonces[j]))
        g1_sx = GF.G1.to_affine(GF.G1.mul(g1_s, secrets[j]))
        pts[nm + "_g1_s"], pts[nm + "_g1_sx"] = g1_s, g1_sx
        pts[nm + "_g2_spx"] = GF.G2.to_affine(GF.G2.mul(derive(challenge, j, g1_s, g1_sx), secrets[j]))
    rec = Record(pts, params=CF.name_params(name))
    rec.next_challenge = H(challenge + rec.pub())
    return rec


def write_section7(records):
    return struct.pack("<I", len(records)) + b"".join(r.stored() for r in records)


def read_section7(body):
    """-> [Record]; well-formed input only"""
    (n,), off, recs = struct.unpack_from("<I", body, 0), 4, []
    for _ in range(n):
        pts, at = {}, off
        for name, g2 in POINTS:
            size = 128 if g2 else 64
            pts[name] = (CF._g2_of if g2 else CF._g1_of)(body[at:at + size])
            at += size
        typ, plen = struct.unpack_from("<II", body, at + 280)
        recs.append(Record(pts, body[at + 216:at + 280], typ, body[at + 288:at + 288 + plen], body[at:at + 216]))
        off = at + 288 + plen
    assert off == len(body)
    return recs
