"""Section 4 of a `.zkey` (the coefficients) written from plain integers, independent of the library's own writer (r1cs/setup.hip):
an entry (matrix, constraint, signal, c) is stored with the value c R^2 mod r, R = 2^256 (snarkjs `zkey new`); the public rows are
(0, nC + i, i, 1) for i = 0 .. nPublic.  Plus the pieces the zkey-only tests share: splicing a section 4 into a zkey, a `.wtns`
image of a row, and the comparison gwb_zkey_check_r1cs makes as dictionary arithmetic."""
import struct

from tests import groth16_fixtures as GF
from tests import r1cs_fixtures as F

R = F.R


def entries_of(constraints, n_pub):
    """(matrix, constraint, signal, coefficient) of the A and B sides of `constraints` (r1cs_fixtures combinations, one entry per
    term, duplicates kept), then the nPublic + 1 public rows"""
    out = []
    for k, (a, b, _) in enumerate(constraints):
        for m, lc in ((0, a), (1, b)):
            out.extend((m, k, wire, co % R) for wire, co in F.terms(lc))
    out.extend((0, len(constraints) + i, i, 1) for i in range(n_pub + 1))
    return out


def section4(entries, count=None):
    """entries: (m, c, s, v); an int v is a coefficient, written as v R^2 mod r; a bytes v is written as it is (32 bytes)"""
    body = [struct.pack("<I", len(entries) if count is None else count)]
    for m, c, s, v in entries:
        raw = v if isinstance(v, bytes) else (v * F.MONT_R2 % R).to_bytes(32, "little")
        assert len(raw) == 32
        body.append(struct.pack("<III", m, c, s) + raw)
    return b"".join(body)


def sections(zkey):
    """zkey bytes -> [(id, body)] in file order"""
    n = struct.unpack_from("<I", zkey, 8)[0]
    off, out = 12, []
    for _ in range(n):
        sid, size = struct.unpack_from("<IQ", zkey, off)
        out.append((sid, zkey[off + 12:off + 12 + size]))
        off += 12 + size
    return out


def join(secs):
    return b"zkey" + struct.pack("<II", 1, len(secs)) + b"".join(GF.section(i, b) for i, b in secs)


def splice(zkey, body4):
    """the zkey with section 4 replaced by the bytes `body4`"""
    return join([(i, body4 if i == 4 else b) for i, b in sections(zkey)])


def zkey_of(trapdoor, entries=None):
    """a Trapdoor's zkey with the section 4 of its own constraints (or of `entries`)"""
    if entries is None:
        entries = entries_of(trapdoor.cons, trapdoor.n_pub)
    return splice(trapdoor.zkey, section4(entries))


def wtns_image(w):
    img = b"wtns" + struct.pack("<II", 2, 2)
    img += struct.pack("<IQ", 1, 40) + struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<I", len(w))
    img += struct.pack("<IQ", 2, 32 * len(w)) + b"".join(x.to_bytes(32, "little") for x in w)
    return img


def summed(entries):
    """{(constraint, matrix, signal): coefficient} with equal keys summed and zero sums dropped"""
    d = {}
    for m, c, s, v in entries:
        d[(c, m, s)] = (d.get((c, m, s), 0) + v) % R
    return {k: v for k, v in d.items() if v}


def first_difference(entries_a, entries_b):
    """the smallest (constraint, matrix, signal) at which the two sums differ, or None"""
    a, b = summed(entries_a), summed(entries_b)
    keys = [k for k in set(a) | set(b) if a.get(k) != b.get(k)]
    return min(keys) if keys else None


def difference_message(key):
    return "zkey: section 4 differs from the r1cs at constraint %d, matrix %s, signal %d" % (key[0], "AB"[key[1]], key[2])
