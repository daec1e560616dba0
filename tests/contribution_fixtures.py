"""Plain-Python phase-2 contribution records for the tests: section 10 of a `.zkey` written and read, the transcript, the
challenge point and a whole record, restated from include/graph_witness_groth16_contribute.h with hashlib's BLAKE2b,
groth16_fixtures.Curve and bn254_pairing.fq2_sqrt (the smaller root chosen as the header defines it)."""
import hashlib
import struct

from tests import bn254_pairing as BP
from tests import groth16_fixtures as GF

R, Q = GF.R, GF.Q
COFACTOR = 2 * Q - R
NO_RECORDS = bytes(64) + struct.pack("<I", 0)


def H(data):
    return hashlib.blake2b(data).digest()


def be(x):
    return x.to_bytes(32, "big")


def U1(p):
    return bytes(64) if p is None else be(p[0]) + be(p[1])


def U2(p):
    return bytes(128) if p is None else be(p[0][1]) + be(p[0][0]) + be(p[1][1]) + be(p[1][0])


def canonical_g1(p):
    return bytes(64) if p is None else p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")


def canonical_g2(p):
    return bytes(128) if p is None else b"".join(x.to_bytes(32, "little") for x in (p[0][0], p[0][1], p[1][0], p[1][1]))


class Record:
    """points affine (None = infinity)"""

    def __init__(self, delta_after, g1_s, g1_sx, g2_spx, transcript, type=0, params=b""):
        self.delta_after, self.g1_s, self.g1_sx, self.g2_spx = delta_after, g1_s, g1_sx, g2_spx
        self.transcript, self.type, self.params = transcript, type, params

    def pub(self):
        return U1(self.delta_after) + U1(self.g1_s) + U1(self.g1_sx) + U2(self.g2_spx) + self.transcript

    def hash(self):
        return H(self.pub())

    def stored(self):
        return (GF.g1_bytes(self.delta_after) + GF.g1_bytes(self.g1_s) + GF.g1_bytes(self.g1_sx) + GF.g2_bytes(self.g2_spx) + self.transcript
                + struct.pack("<II", self.type, len(self.params)) + self.params)


def name_params(name):
    nm = name.encode("utf-8")
    return bytes([1, len(nm)]) + nm if nm else b""


def beacon_params(name, iterations_exp, beacon_hash):
    return name_params(name) + bytes([2, iterations_exp]) + bytes([3, len(beacon_hash)]) + beacon_hash


def write_section10(cs_hash, records):
    return cs_hash + struct.pack("<I", len(records)) + b"".join(r.stored() for r in records)


def _fq_of(b):
    return int.from_bytes(b, "little") * pow(GF.MONT, -1, Q) % Q


def _g1_of(b):
    return None if not any(b) else (_fq_of(b[:32]), _fq_of(b[32:64]))


def _g2_of(b):
    return None if not any(b) else ((_fq_of(b[:32]), _fq_of(b[32:64])), (_fq_of(b[64:96]), _fq_of(b[96:128])))


def read_section10(body):
    """-> (cs_hash, [Record]); well-formed input only"""
    cs_hash, (n,) = body[:64], struct.unpack_from("<I", body, 64)
    off, recs = 68, []
    for _ in range(n):
        typ, plen = struct.unpack_from("<II", body, off + 384)
        recs.append(Record(_g1_of(body[off:off + 64]), _g1_of(body[off + 64:off + 128]), _g1_of(body[off + 128:off + 192]),
                           _g2_of(body[off + 192:off + 320]), body[off + 320:off + 384], typ, body[off + 392:off + 392 + plen]))
        off += 392 + plen
    assert off == len(body)
    return cs_hash, recs


def transcript(cs_hash, before, g1_s, g1_sx):
    return H(cs_hash + b"".join(r.pub() for r in before) + U1(g1_s) + U1(g1_sx))


def smaller_root(y):
    ny = GF.Fq2.neg(y)
    return min(y, ny, key=lambda v: (v[1], v[0]))


def hash_to_g2_trace(t):
    """-> (point, [why each rejected counter was rejected])"""
    F2, why, ctr = GF.Fq2, [], 0
    while True:
        d = H(t + b"cwc-g2" + struct.pack("<I", ctr))
        ctr += 1
        c0 = int.from_bytes(d[:32], "little") & ((1 << 254) - 1)
        c1 = int.from_bytes(d[32:], "little") & ((1 << 254) - 1)
        if c0 >= Q or c1 >= Q:
            why.append("range")
            continue
        x = (c0, c1)
        y = BP.fq2_sqrt(F2.add(F2.mul(F2.mul(x, x), x), GF.B2))
        if y is None:
            why.append("square")
            continue
        p = GF.G2.to_affine(GF.G2.mul((x, smaller_root(y)), COFACTOR))
        if p is None:
            why.append("infinity")
            continue
        return p, why


def hash_to_g2(t):
    return hash_to_g2_trace(t)[0]


def contribution(cs_hash, before, delta_prev, delta, s, name=""):
    """the record a contribution with secret delta and nonce s appends after `before`, delta_prev the key's delta1 (affine)"""
    g1_s = GF.G1.to_affine(GF.G1.gen_mul_jac(s))
    g1_sx = GF.G1.to_affine(GF.G1.mul(g1_s, delta))
    t = transcript(cs_hash, before, g1_s, g1_sx)
    g2_spx = GF.G2.to_affine(GF.G2.mul(hash_to_g2(t), delta))
    return Record(GF.G1.to_affine(GF.G1.mul(delta_prev, delta)), g1_s, g1_sx, g2_spx, t, 0, name_params(name))
