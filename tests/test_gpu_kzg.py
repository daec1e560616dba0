"""KZG commitments over a powers-of-tau file on an MI355X (include/graph_witness_kzg.h): commit, commit_evals, open and verify on
a power-4 and a power-9 file that the device makes from a known tau (ptau_contribute on ptau_new, then ptau_prepare_phase2), with
max_len = 2^(power+1) - 1.  With tau known the oracle of a commitment is one fixed-base product on the plain-Python curve,
p(tau) G1; the oracle of y and of the quotient is synchronous division on Python integers; no Python pairing is needed: honest
rows are made from tau alone, and every wrong row is wrong by construction.

Wall time on an MI355X: the module's files and the Python curve's table about 2 s once; each test well under a second but the
first commit test (the table) at 2 s, the CLI's three processes at 1.5 s and the child process of the sub-batch test at 3 s."""
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import cwc_import
from tests import groth16_fixtures as GF
from tests import kzg_model as M
from tests import qap_reference as QR

PKG = cwc_import.load()
R, Q = GF.R, GF.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "circom-witnesscalc_amd", "kzg")
TAU = random.Random(2024).randrange(2, R)
POWERS = (4, 9)
V, S, P, E = PKG.KZG_VALID, PKG.KZG_SCALAR, PKG.KZG_POINT, PKG.KZG_EQUATION

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def ptau(power, prepared=False):
    if prepared:
        return PKG.ptau_prepare_phase2(ptau(power))
    return PKG.ptau_contribute(PKG.ptau_new(power), secrets=(TAU, 1, 1))[0]


@functools.lru_cache(maxsize=None)
def kzg(power, prepared=False):
    return PKG.Kzg(ptau(power, prepared))


def le(values):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), dtype=np.uint8)


def scalars(values):
    return le(values).reshape(len(values), 32).copy()


def rows(polys):
    """[K lists of N ints] -> uint8 [K, N, 32]"""
    return np.stack([le(p) for p in polys]).reshape(len(polys), len(polys[0]), 32).copy()


def pt(p):
    """an affine point of the Python curve (None: infinity) -> the 64 canonical bytes"""
    return bytes(64) if p is None else p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little")


def points(logs):
    """[k] -> uint8 [K, 64] of k G1"""
    return np.frombuffer(b"".join(pt(p) for p in GF.G1.gen_muls([k % R for k in logs])), dtype=np.uint8).reshape(len(logs), 64).copy()


def at_tau(c):
    return M.horner([x % R for x in c], TAU)[0]


def opening(c, z):
    """(log of C, y, log of W) of the honest opening of c at z, from tau alone"""
    y, q = M.horner([x % R for x in c], z % R)
    return at_tau(c), y, at_tau(q)


# -- commit -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", POWERS)
def test_commit_is_p_of_tau_times_g1(power):
    rnd = random.Random(power)
    k = kzg(power)
    max_len = (2 << power) - 1
    assert k.info == {"max_len": max_len, "power": power, "prepared": False}
    for n in (1, 2, max_len):
        polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(3)]  # K = 3 in one call
        polys[1][0] = R + 7  # reduced
        assert np.array_equal(k.commit(rows(polys)), points([at_tau(p) for p in polys])), n
    assert np.array_equal(k.commit(np.zeros((2, 0, 32), dtype=np.uint8)), np.zeros((2, 64), dtype=np.uint8))  # N = 0
    assert not k.commit(np.zeros((1, max_len, 32), dtype=np.uint8)).any()  # the zero polynomial
    one = k.commit(rows([[1]]))
    assert bytes(one[0]) == pt(GF.G1_GEN)


@pytest.mark.parametrize("m", (1, 4))
def test_commit_evals_is_commit_of_the_polynomial(m):
    rnd = random.Random(m)
    n = 1 << m
    w = QR.roots(m)[0]
    polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(3)]
    evals = [[M.horner(p, pow(w, i, R))[0] for i in range(n)] for p in polys]
    k = kzg(4, True)
    assert k.info["prepared"]
    got = k.commit_evals(rows(evals))
    assert np.array_equal(got, k.commit(rows(polys))) and np.array_equal(got, points([at_tau(p) for p in polys]))


# -- open -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", POWERS)
def test_open_gives_pythons_y_and_the_quotient_at_tau(power):
    rnd = random.Random(10 + power)
    k = kzg(power)
    max_len = (2 << power) - 1
    for n in (1, 2, 17, max_len):
        polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(4)]
        zs = [rnd.randrange(R), 0, TAU, R - 1]
        want = [opening(p, z) for p, z in zip(polys, zs)]
        ys, ws = k.open(rows(polys), scalars(zs))
        assert np.array_equal(ys, scalars([y for _, y, _ in want])), n
        assert np.array_equal(ws, points([w for _, _, w in want])), n
        assert np.array_equal(k.eval(rows(polys), scalars(zs)), ys)
        if n == 1:
            assert not ws.any()  # W is the point at infinity
    ph = PKG.kzg_phase_ms(k)
    assert set(ph) == {"quotient", "lincomb", "prepare", "pairing"} and ph["quotient"] > 0 and ph["lincomb"] > 0 and ph["prepare"] == 0 == ph["pairing"]
    ys, ws = k.open(np.zeros((2, 0, 32), dtype=np.uint8), scalars([5, 6]))
    assert not ys.any() and not ws.any()


# -- verify -----------------------------------------------------------------------------------------------------------------------
def honest(rnd, count, n=8):
    """`count` honest rows of one random polynomial of n coefficients at random points, from tau alone: (C, z, y, W) arrays"""
    p = [rnd.randrange(R) for _ in range(n)]
    zs = [rnd.randrange(R) for _ in range(count)]
    ops = [opening(p, z) for z in zs]
    return points([ops[0][0]] * count), scalars(zs), scalars([y for _, y, _ in ops]), points([w for _, _, w in ops])


@pytest.mark.parametrize("count", (65, 257))
def test_one_bad_row_at_the_end_of_a_batch(count):
    rnd = random.Random(count)
    c, z, y, w = honest(rnd, count)
    bad = int.from_bytes(bytes(y[-1]), "little")
    y[-1] = scalars([(bad + 1) % R])[0]
    got = kzg(4).verify(c, z, y, w)
    assert got.dtype == np.uint32 and list(got) == [V] * (count - 1) + [E]
    ph = PKG.kzg_phase_ms(kzg(4))
    assert ph["prepare"] > 0 and ph["pairing"] > 0 and ph["quotient"] == 0 == ph["lincomb"]


def mixed_rows(power):
    """[(name, C, z, y, W, status)] with C and W as 64 bytes and z, y as ints"""
    rnd = random.Random(100 + power)
    k = kzg(power)
    n = (2 << power) - 1
    p = [rnd.randrange(R) for _ in range(n)]
    z = rnd.randrange(R)
    lc, y, lw = opening(p, z)
    C, W = pt(GF.G1.gen_muls([lc])[0]), pt(GF.G1.gen_muls([lw])[0])
    out = []
    ys, ws = k.open(rows([p]), scalars([z]))
    cs = k.commit(rows([p]))
    out.append(("made by open", bytes(cs[0]), z, int.from_bytes(bytes(ys[0]), "little"), bytes(ws[0]), V))
    out.append(("made from tau alone", C, z, y, W, V))
    out.append(("the zero polynomial with y = 0", bytes(64), z, 0, bytes(64), V))
    const = rnd.randrange(1, R)
    Cc = pt(GF.G1.gen_muls([const])[0])
    out.append(("a constant polynomial", Cc, z, const, bytes(64), V))
    lct, yt, lwt = opening(p, TAU)
    out.append(("z = tau", C, TAU, yt, pt(GF.G1.gen_muls([lwt])[0]), V))
    assert yt == lc
    out.append(("y + 1", C, z, (y + 1) % R, W, E))
    out.append(("z + 1", C, (z + 1) % R, y, W, E))
    out.append(("2 C", pt(GF.G1.gen_muls([2 * lc])[0]), z, y, W, E))
    out.append(("a W with log q(tau) + 1", C, z, y, pt(GF.G1.gen_muls([lw + 1])[0]), E))
    out.append(("a constant polynomial with the wrong y", Cc, z, (const + 1) % R, bytes(64), E))
    out.append(("W at infinity for a polynomial that is not constant", C, z, y, bytes(64), E))
    out.append(("y = r", C, z, R, W, S))
    out.append(("z = r", C, R, y, W, S))
    off = C[:32] + ((int.from_bytes(C[32:], "little") + 1) % Q).to_bytes(32, "little")
    out.append(("a C off the curve", off, z, y, W, P))
    out.append(("a coordinate equal to q", Q.to_bytes(32, "little") + C[32:], z, y, W, P))
    out.append(("a W off the curve", C, z, y, W[:32] + bytes(31) + b"\x01", P))
    out.append(("y = r and a C off the curve: the scalar rule is first", off, z, R, W, S))
    out.append(("a C off the curve and a wrong y: the point rule is first", off, z, (y + 1) % R, W, P))
    return out


def arrays(rws):
    c = np.frombuffer(b"".join(r[1] for r in rws), dtype=np.uint8).reshape(-1, 64).copy()
    w = np.frombuffer(b"".join(r[4] for r in rws), dtype=np.uint8).reshape(-1, 64).copy()
    return c, scalars([r[2] for r in rws]), scalars([r[3] for r in rws]), w


@pytest.mark.parametrize("power", POWERS)
def test_every_row_kind_in_one_mixed_batch(power):
    rws = mixed_rows(power)
    got = kzg(power).verify(*arrays(rws))
    assert {r[0]: int(g) for r, g in zip(rws, got)} == {r[0]: r[5] for r in rws}


# -- the twins, the CLI -----------------------------------------------------------------------------------------------------------
def test_host_and_device_twins_agree():
    import torch
    rnd = random.Random(31)
    k = kzg(4, True)
    polys = rows([[rnd.randrange(R) for _ in range(16)] for _ in range(3)])
    zs = scalars([rnd.randrange(R) for _ in range(3)])
    d_polys, d_zs = torch.from_numpy(polys).cuda(), torch.from_numpy(zs).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    d_c = k.commit_device(d_polys, stream=s)
    d_ce = k.commit_evals_device(d_polys, stream=s)
    d_ys, d_ws = k.open_device(d_polys, d_zs, stream=s)
    d_st = k.verify_device(d_c, d_zs, d_ys, d_ws, stream=s)
    d_bad = k.verify_device(d_ce, d_zs, d_ys, d_ws, stream=s)  # (one stream: the handle's workspace is one)
    s.synchronize()
    torch.cuda.synchronize()
    c, (ys, ws) = k.commit(polys), k.open(polys, zs)
    assert np.array_equal(d_c.cpu().numpy(), c) and np.array_equal(d_ce.cpu().numpy(), k.commit_evals(polys))
    assert np.array_equal(d_ys.cpu().numpy(), ys) and np.array_equal(d_ws.cpu().numpy(), ws)
    assert d_st.dtype == torch.int32 and list(d_st.cpu().numpy()) == [V] * 3 == list(k.verify(c, zs, ys, ws))
    assert list(d_bad.cpu().numpy()) == list(k.verify(d_ce.cpu().numpy(), zs, ys, ws))


def test_the_cli_round_trip(tmp_path):
    rnd = random.Random(41)
    names = ("pot.ptau", "poly.bin", "z.bin", "c.bin", "y.bin", "w.bin")
    pot, poly, z, c, y, w = (tmp_path / n for n in names)
    pot.write_bytes(ptau(4))
    p, zz = [rnd.randrange(R) for _ in range(20)], rnd.randrange(R)
    poly.write_bytes(bytes(le(p)))
    z.write_bytes(zz.to_bytes(32, "little"))
    run = lambda *a: subprocess.run([CLI] + [str(x) for x in a], capture_output=True, text=True)  # noqa: E731
    r = run("commit", pot, poly, c)
    assert r.returncode == 0, r.stderr
    r = run("open", pot, poly, z, y, w)
    assert r.returncode == 0, r.stderr
    lc, yy, lw = opening(p, zz)
    assert c.read_bytes() == bytes(points([lc])[0]) and y.read_bytes() == yy.to_bytes(32, "little") and w.read_bytes() == bytes(points([lw])[0])
    r = run("verify", pot, c, z, y, w)
    assert r.returncode == 0 and r.stdout.strip() == "OK!", (r.stdout, r.stderr)
    flipped = bytearray(y.read_bytes())
    flipped[0] ^= 1
    y.write_bytes(bytes(flipped))
    r = run("verify", pot, c, z, y, w)
    assert r.returncode == 1 and r.stdout.strip() == "EQUATION", (r.stdout, r.stderr)


CHILD = """
import sys
import numpy as np
import cwc_import
pkg = cwc_import.load()
k = pkg.Kzg(open(sys.argv[1], "rb").read())
a = np.load(sys.argv[2])
ys, ws = k.open(a["polys"], a["zs"])
st = k.verify(a["c"], a["vz"], a["vy"], a["vw"])
np.savez(sys.argv[3], ys=ys, ws=ws, st=st)
"""


def test_sub_batches_under_a_small_workspace_cap(tmp_path):
    """CWC_GROTH16_WORKSPACE_MB is read once per process, so a child process runs under 1 MB: 40 openings of 1 023 coefficients
    (32 KB of quotient each) are two sub-batches, and 257 checked rows (8.7 KB each with their pairings' workspace) are three.
    The results are those of this process, whose cap is the default."""
    rnd = random.Random(51)
    polys = rows([[rnd.randrange(R) for _ in range(1023)] for _ in range(40)])
    zs = scalars([rnd.randrange(R) for _ in range(40)])
    c, vz, vy, vw = honest(rnd, 257)
    vy[100] = scalars([5])[0]
    (tmp_path / "pot.ptau").write_bytes(ptau(9))
    np.savez(tmp_path / "in.npz", polys=polys, zs=zs, c=c, vz=vz, vy=vy, vw=vw)
    env = dict(os.environ, CWC_GROTH16_WORKSPACE_MB="1")
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "pot.ptau"), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env, cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.load(tmp_path / "out.npz")
    ys, ws = kzg(9).open(polys, zs)
    assert np.array_equal(got["ys"], ys) and np.array_equal(got["ws"], ws)
    assert list(got["st"]) == [E if i == 100 else V for i in range(257)] == list(kzg(9).verify(c, vz, vy, vw))


def test_check_powers_accepts_the_ceremonys_file():
    k = PKG.Kzg(ptau(4), max_len=9, check_powers=True)  # the domain 2^3 covers 9 points
    assert k.info["max_len"] == 9
    whole = PKG.Kzg(ptau(4), check_powers=True)  # 31 points: the whole file's sums
    assert whole.info["max_len"] == 31
