"""The Groth16 prover's host side without a GPU: the plain-Python BN254 of tests/groth16_fixtures.py (curve equations, group
orders, the twist constant, the trapdoor identity behind the H points), the `.zkey` loader (round trip, every refusal, a
mutant fuzz), the groth16-prove CLI's usage errors, and the Fq product generator against the committed .inc."""
import os
import random
import struct
import subprocess
import sys

import pytest

import cwc_import
from tests import groth16_fixtures as GF
from tests import qap_reference as QR
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, Q = GF.R, GF.Q


# -- fixture arithmetic ---------------------------------------------------------------------------------------------------------
def test_generators_on_curve_with_order_r():
    assert GF.G1.on_curve(GF.G1_GEN) and GF.G2.on_curve(GF.G2_GEN)
    assert GF.G1.is_inf(GF.G1.mul(GF.G1_GEN, R))
    assert GF.G2.is_inf(GF.G2.mul(GF.G2_GEN, R))
    assert not GF.G2.is_inf(GF.G2.mul(GF.G2_GEN, R - 1))


def test_twist_constant():
    assert GF.Fq2.mul(GF.B2, (9, 1)) == (3, 0)
    # the published coordinates of 3 / (9 + u)
    assert GF.B2 == (19485874751759354771024239261021720505790618469301721065564631296452457478373,
                     266929791119991161246907387137283842545076965332900288569378510910307636690)


def test_fixed_base_table_matches_double_and_add():
    for k in (0, 1, 2, 255, 256, R - 1, random.Random(4).randrange(R)):
        assert GF.G1.to_affine(GF.G1.gen_mul_jac(k)) == GF.G1.to_affine(GF.G1.mul(GF.G1_GEN, k))
        assert GF.G2.to_affine(GF.G2.gen_mul_jac(k)) == GF.G2.to_affine(GF.G2.mul(GF.G2_GEN, k))


def _planted(seed, n_constraints, n_pub_out=1, n_pub_in=2):
    rnd = random.Random(seed)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(n_constraints)]
    pl = F.planted_system(rnd, 5, shapes, [1, R - 1, 2, None])
    return rnd, pl, n_pub_out + n_pub_in


@pytest.mark.parametrize("n_constraints", [1, 5, 12])
def test_trapdoor_identity(n_constraints):
    """sum_j h_j L^2n_{2j+1}(tau) = A(tau) B(tau) - C(tau) (C from c_k = a_k b_k), and a satisfied row verifies"""
    rnd, pl, n_pub = _planted(n_constraints, n_constraints)
    w = pl.complete(rnd)
    # the identity itself, over the domain of the system
    a, b, c = QR.qap_rows(pl.constraints, n_pub, w)
    h = QR.h_ntt(a, b, c)
    n = len(a)
    wn, g = QR.roots(n.bit_length() - 1)
    tau = rnd.randrange(R)
    zf = (pow(tau, n, R) - 1) * pow(n, -1, R) % R
    lag = [zf * pow(wn, k, R) * pow(tau - pow(wn, k, R), -1, R) % R for k in range(n)]
    ev = lambda v: sum(x * y for x, y in zip(v, lag)) % R  # noqa: E731
    zf2 = (pow(tau, 2 * n, R) - 1) * pow(2 * n, -1, R) % R
    lh = [zf2 * g * pow(wn, j, R) * pow(tau - g * pow(wn, j, R), -1, R) % R for j in range(n)]
    assert sum(x * y for x, y in zip(h, lh)) % R == (ev(a) * ev(b) - ev(c)) % R
    # the verification equation on the logs of a trapdoor zkey
    T = GF.Trapdoor(pl.constraints, pl.n_wires, n_pub, seed=n_constraints)
    r_, s_ = rnd.randrange(R), rnd.randrange(R)
    assert T.verifies(w, *T.proof_logs(w, r_, s_))
    bad = list(w)
    bad[-1] = (bad[-1] + 1) % R
    if F.check(pl.constraints, bad)[1]:
        assert not T.verifies(bad, *T.proof_logs(bad, r_, s_))


# -- the loader ---------------------------------------------------------------------------------------------------------------
def _small_zkey(**kw):
    _, pl, n_pub = _planted(7, 4)
    T = GF.Trapdoor(pl.constraints, pl.n_wires, n_pub, seed=2)
    return T, pl


def _sections(data):
    """zkey bytes -> [(id, body)]"""
    n = struct.unpack_from("<I", data, 8)[0]
    off, out = 12, []
    for _ in range(n):
        sid, size = struct.unpack_from("<IQ", data, off)
        out.append((sid, data[off + 12:off + 12 + size]))
        off += 12 + size
    return out


def _join(secs, version=1):
    return b"zkey" + struct.pack("<II", version, len(secs)) + b"".join(GF.section(i, b) for i, b in secs)


def _load(data):
    return PKG.Groth16(data, PKG.R1cs(F.write_r1cs(3, [([(0, 1)], [(0, 1)], [(0, 1)])])))


def test_round_trip_and_info():
    T, pl = _small_zkey()
    g = _load(T.zkey)
    assert g.info == {"n_vars": pl.n_wires, "n_public": T.n_pub, "domain_size": T.n, "n_coefs": 0}
    # sections in another order, a contributions section and a section id the loader ignores
    secs = _sections(T.zkey)
    secs = secs[::-1] + [(11, b"xyz")]
    assert _load(_join(secs)).info == g.info


def _refused(data, fragment):
    with pytest.raises(PKG.WitnessCalcError, match=fragment):
        _load(data)


def test_refusals():
    T, pl = _small_zkey()
    z = T.zkey
    secs = _sections(z)
    by = dict(secs)
    _refused(b"zkex" + z[4:], "bad magic")
    _refused(z[:4] + struct.pack("<I", 2) + z[8:], "version")
    for proto, name in ((2, "PLONK"), (10, "fflonk"), (7, "unknown protocol")):
        _refused(_join([(1, struct.pack("<I", proto)) if i == 1 else (i, b) for i, b in secs]), name)
    hdr = by[2]
    bad_q = struct.pack("<I", 32) + (Q + 2).to_bytes(32, "little") + hdr[36:]
    _refused(_join([(2, bad_q) if i == 2 else (i, b) for i, b in secs]), "base field q")
    bad_r = hdr[:40] + (R + 2).to_bytes(32, "little") + hdr[72:]
    _refused(_join([(2, bad_r) if i == 2 else (i, b) for i, b in secs]), "scalar field r")
    _refused(_join([(2, struct.pack("<I", 48) + hdr[4:]) if i == 2 else (i, b) for i, b in secs]), "n8q")
    _refused(_join([(2, hdr[:36] + struct.pack("<I", 48) + hdr[40:]) if i == 2 else (i, b) for i, b in secs]), "n8r")
    _refused(z[:-5], "truncated")
    _refused(z + b"\0", "trailing")
    for sid in range(1, 10):
        _refused(_join([(i, b) for i, b in secs if i != sid]), "missing section %d" % sid)
    _refused(_join(secs + [(5, by[5])]), "duplicate section 5")
    _refused(_join([(5, by[5][:-64]) if i == 5 else (i, b) for i, b in secs]), r"section 5 \(A\)")
    _refused(_join([(9, by[9] + bytes(64)) if i == 9 else (i, b) for i, b in secs]), r"section 9 \(H\)")
    non_pow2 = hdr[:80] + struct.pack("<I", T.n + 1) + hdr[84:]
    _refused(_join([(2, non_pow2) if i == 2 else (i, b) for i, b in secs]), "power of two")
    # a coordinate >= q; points off their curves
    a = bytearray(by[5])
    a[0:32] = (Q + 1).to_bytes(32, "little")
    _refused(_join([(5, bytes(a)) if i == 5 else (i, b) for i, b in secs]), ">= q")
    a = bytearray(by[5])
    a[32:64] = GF.lem(5)
    _refused(_join([(5, bytes(a)) if i == 5 else (i, b) for i, b in secs]), "not on the G1 curve")
    b2 = bytearray(by[7])
    b2[96:128] = GF.lem(5)
    _refused(_join([(7, bytes(b2)) if i == 7 else (i, b) for i, b in secs]), "not on the G2 curve")
    # section 4 bounds
    s4 = lambda m, k, s: struct.pack("<I", 1) + struct.pack("<III", m, k, s) + bytes(32)  # noqa: E731
    _refused(_join([(4, s4(2, 0, 0)) if i == 4 else (i, b) for i, b in secs]), "matrix")
    _refused(_join([(4, s4(0, T.n, 0)) if i == 4 else (i, b) for i, b in secs]), "constraint")
    _refused(_join([(4, s4(1, 0, pl.n_wires)) if i == 4 else (i, b) for i, b in secs]), "signal")
    _refused(_join([(4, struct.pack("<I", 2) + bytes(44)) if i == 4 else (i, b) for i, b in secs]), "section 4")
    assert _load(_join([(4, s4(1, T.n - 1, pl.n_wires - 1)) if i == 4 else (i, b) for i, b in secs])).info["n_coefs"] == 1


def test_mutant_fuzz():
    """single-byte mutations and truncations of a valid zkey: loaded or refused with a message, never a crash"""
    T, _ = _small_zkey()
    z = T.zkey
    rnd = random.Random(11)
    refused = 0
    for _ in range(300):
        m = bytearray(z)
        for _ in range(rnd.randrange(1, 4)):
            m[rnd.randrange(len(m))] = rnd.randrange(256)
        if rnd.random() < 0.2:
            m = m[:rnd.randrange(len(m))]
        try:
            _load(bytes(m))
        except PKG.WitnessCalcError as e:
            assert str(e).startswith("zkey:")
            refused += 1
    assert refused > 200


def test_cli_usage_errors(tmp_path):
    cli = os.path.join(ROOT, "circom-witnesscalc_amd", "groth16-prove")
    assert subprocess.run([cli], capture_output=True).returncode == 2
    p = subprocess.run([cli, str(tmp_path / "no.r1cs"), "b", "c", "d", "e"], capture_output=True, text=True)
    assert p.returncode == 2 and "cannot read" in p.stderr
    r1 = tmp_path / "c.r1cs"
    r1.write_bytes(F.write_r1cs(3, [([(0, 1)], [(0, 1)], [(0, 1)])]))
    zk = tmp_path / "c.zkey"
    zk.write_bytes(b"zkey" + bytes(8))
    wt = tmp_path / "w.wtns"
    wt.write_bytes(b"")
    p = subprocess.run([cli, str(r1), str(zk), str(wt), str(tmp_path / "p.json"), str(tmp_path / "q.json")], capture_output=True, text=True)
    assert p.returncode == 2 and "zkey:" in p.stderr


def test_fq_generator_reproduces_the_committed_inc(tmp_path):
    out = tmp_path / "fq.inc"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "codegen", "gen_fq_mul.py"), str(out)], stdout=subprocess.DEVNULL)
    committed = os.path.join(ROOT, "circom-witnesscalc_amd", "r1cs", "fq_mul_gfx950.inc")
    assert out.read_bytes() == open(committed, "rb").read()
