"""Folded KZG openings on an MI355X (include/graph_witness_kzg.h): the fold kernel and the verifier's point fold alone, open_fold
and verify_fold on the power-4 and power-9 files of tests/test_gpu_kzg.py (made on the device from a known tau), the host and
device twins, sub-batches and the CLI.  The oracles are bytes from plain integers (tests/kzg_fold_model.py) and the plain-Python
curve: with tau known a commitment or a witness is its polynomial's value at tau times G1, so every honest group is made from tau
alone and every wrong group is wrong by construction.  Everything is compared exactly."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import cwc_import
from tests import groth16_fixtures as GF
from tests import kzg_fold_model as FM
from tests import test_gpu_kzg as T

PKG = cwc_import.load()
R, Q = GF.R, GF.Q
ROOT, CLI, TAU, POWERS = T.ROOT, T.CLI, T.TAU, T.POWERS
V, S, P, E = PKG.KZG_VALID, PKG.KZG_SCALAR, PKG.KZG_POINT, PKG.KZG_EQUATION
le, scalars, pt, points, kzg, ptau = T.le, T.scalars, T.pt, T.points, T.kzg, T.ptau
GAMMAS = (0, 1, R - 1, R + 5, random.Random(3).randrange(R))

pytestmark = pytest.mark.gpu


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def groups(gs):
    """[G groups of K lists of N ints] -> uint8 [G, K, N, 32]"""
    return np.stack([T.rows(g) for g in gs]) if len(gs[0][0]) else np.zeros((len(gs), len(gs[0]), 0, 32), dtype=np.uint8)


def values(vs):
    """[G lists of K ints] -> uint8 [G, K, 32]"""
    return np.stack([scalars(v) for v in vs])


def point_rows(logs):
    """[G lists of K logs] -> uint8 [G, K, 64]"""
    return points([x for g in logs for x in g]).reshape(len(logs), len(logs[0]), 64)


def random_groups(rnd, g, k, n):
    return [[[rnd.randrange(R) for _ in range(n)] for _ in range(k)] for _ in range(g)]


def single_row_times(k, verify):
    """kzg_phase_ms after a single-row call, a verify or an open: what a folded call has to leave alone"""
    if verify:
        k.verify(points([5]), scalars([3]), scalars([5]), np.zeros((1, 64), dtype=np.uint8))
    else:
        k.open(T.rows([[1, 2]]), scalars([3]))
    return PKG.kzg_phase_ms(k)


def same_times(k, before):
    """the handle's single-row times are those of `before`: the same phases are 0, and the others are the same events read again
    (two readings of one pair of events differ in the last digits)"""
    now = PKG.kzg_phase_ms(k)
    return all((now[n] == 0) == (before[n] == 0) and now[n] == pytest.approx(before[n], rel=1e-3) for n in PKG.KZG_PHASES)


# -- the fold kernel alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 255, 256, 257, 1025))
def test_the_fold_kernel(n):
    rnd = random.Random(n)
    for i, k in enumerate((1, 2, 3, 17)):
        gs = random_groups(rnd, 3, k, n)
        gs[0][0][0] = R + 7  # reduced on load
        gs[2][k - 1][n - 1] = (1 << 256) - 1
        gammas = [GAMMAS[(i + n + j) % 5] for j in range(3)]  # every gamma of GAMMAS over the cases
        got = PKG.kzg_fold_device(cuda(groups(gs)), cuda(scalars(gammas))).cpu().numpy()
        assert np.array_equal(got, T.rows([FM.fold(g, gamma) for g, gamma in zip(gs, gammas)])), (n, k)


def test_the_fold_kernel_with_every_gamma_in_one_call():
    rnd = random.Random(5)
    gs = random_groups(rnd, 5, 3, 300)
    got = PKG.kzg_fold_device(cuda(groups(gs)), cuda(scalars(list(GAMMAS)))).cpu().numpy()
    assert np.array_equal(got, T.rows([FM.fold(g, gamma) for g, gamma in zip(gs, GAMMAS)]))


# -- the point fold alone -------------------------------------------------------------------------------------------------------------
def corner_logs(rnd, k):
    """[(logs of C_0 .. C_{K-1}, gamma)]: a random group; an infinity and a doubling inside an addition (C_0 = C_1, and C_32 = C_0,
    which meets C_0 in the tree's first step); C_1 = -C_0 and C_32 = -C_0, sums that are O in the middle of the tree; a whole
    group that sums to O"""
    out = [([rnd.randrange(R) for _ in range(k)], rnd.randrange(R))]
    dbl = [rnd.randrange(1, R) for _ in range(k)]
    neg = [rnd.randrange(1, R) for _ in range(k)]
    if k > 1:
        dbl[1], neg[1] = dbl[0], R - neg[0]
    if k > 2:
        dbl[2] = 0
    if k > 32:
        dbl[32], neg[32] = dbl[0], R - neg[0]
    out += [(dbl, 1), (neg, 1)]
    gamma = rnd.randrange(2, R)
    zero = [rnd.randrange(R) for _ in range(k)]
    zero[k - 1] = 0
    zero[k - 1] = (R - FM.fold_values(zero, gamma)) * pow(gamma, -(k - 1), R) % R
    assert FM.fold_values(zero, gamma) == 0
    return out + [(zero, gamma), ([0] * k, R + 3)]


@pytest.mark.parametrize("k", (1, 2, 3, 63, 64, 65, 129))
def test_the_point_fold(k):
    cases = corner_logs(random.Random(k), k)
    got = PKG.kzg_fold_points_device(cuda(point_rows([c for c, _ in cases])), cuda(scalars([g for _, g in cases]))).cpu().numpy()
    assert np.array_equal(got, points([FM.fold_values(c, g % R) for c, g in cases]))
    assert not got[3].any() and not got[4].any()


def test_the_point_fold_refuses_a_wrong_point():
    rnd = random.Random(9)
    cs = point_rows([[rnd.randrange(1, R) for _ in range(70)] for _ in range(3)])
    cs[1, 69, 32] ^= 1  # off the curve, in the second chunk of group 1
    with pytest.raises(PKG.WitnessCalcError, match=r"^kzg: a point of group 1 has a coordinate at or above q, or is neither on the curve"):
        PKG.kzg_fold_points_device(cuda(cs), cuda(scalars([1, 2, 3])))


# -- open_fold ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", POWERS)
def test_open_fold_gives_pythons_values_and_the_folded_quotient_at_tau(power):
    rnd = random.Random(20 + power)
    k = kzg(power)
    max_len = (2 << power) - 1
    before = None
    for i, n in enumerate((1, 2, 17, max_len)):
        gs = random_groups(rnd, 3, 4, n)
        gs[1][2][0] = R + 7
        zs = [(0, TAU, R - 1, rnd.randrange(R))[(i + j) % 4] for j in range(3)]
        gammas = [GAMMAS[(i + j + 2) % 5] for j in range(3)]
        want = [FM.logs(g, z, gamma, TAU) for g, z, gamma in zip(gs, zs, gammas)]
        if before is None:
            before = single_row_times(k, verify=True)  # an open_fold that wrote them would leave prepare and pairing 0
        ys, ws = k.open_fold(groups(gs), scalars(zs), scalars(gammas))
        assert np.array_equal(ys, values([y for _, y, _ in want])), n
        assert np.array_equal(ws, points([w for _, _, w in want])), n
        if n == 1:
            assert not ws.any()
    ph = PKG.kzg_fold_phase_ms(k)
    assert tuple(ph) == PKG.KZG_FOLD_PHASES and all(ph[x] > 0 for x in ("fold", "evals", "quotient", "lincomb")) and ph["prepare"] == 0 == ph["pairing"]
    assert before["prepare"] > 0 and same_times(k, before)  # the single-row call's times are not touched
    ys, ws = k.open_fold(np.zeros((2, 3, 0, 32), dtype=np.uint8), scalars([5, 6]), scalars([7, 8]))  # N = 0
    assert ys.shape == (2, 3, 32) and not ys.any() and ws.shape == (2, 64) and not ws.any()


@pytest.mark.parametrize("power", POWERS)
def test_one_polynomial_per_group_is_open_byte_for_byte(power):
    rnd = random.Random(30 + power)
    k = kzg(power)
    for n in (1, 17, (2 << power) - 1):
        polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(5)]
        polys[3][n - 1] = R + 1
        zs = scalars([rnd.randrange(R), 0, TAU, R + 2, R - 1])
        ys, ws = k.open(T.rows(polys), zs)
        fys, fws = k.open_fold(T.rows(polys).reshape(5, 1, n, 32), zs, scalars(list(GAMMAS)))
        assert np.array_equal(fys.reshape(5, 32), ys) and np.array_equal(fws, ws), n


# -- verify_fold ----------------------------------------------------------------------------------------------------------------------
def honest(rnd, count, k, n=8):
    """`count` honest groups of the same k random polynomials at random points and challenges, from tau alone"""
    polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(k)]
    zs, gammas = [rnd.randrange(R) for _ in range(count)], [rnd.randrange(R) for _ in range(count)]
    ops = [FM.logs(polys, z, gamma, TAU) for z, gamma in zip(zs, gammas)]
    c = np.broadcast_to(points(ops[0][0]), (count, k, 64)).copy()
    return c, scalars(zs), scalars(gammas), values([y for _, y, _ in ops]), points([w for _, _, w in ops])


def bump(arr, index):
    """arr[index], a scalar, plus one mod r"""
    arr[index] = scalars([(int.from_bytes(bytes(arr[index]), "little") + 1) % R])[0]


def mixed_groups(power, K=3):
    """[(name, [C_k] as 64 bytes each, z, gamma, [y_k], W as 64 bytes, status)]"""
    rnd = random.Random(200 + power)
    k = kzg(power)
    n = (2 << power) - 1
    polys = random_groups(rnd, 1, K, n)[0]
    z, gamma = rnd.randrange(R), rnd.randrange(2, R)
    lcs, ys, lw = FM.logs(polys, z, gamma, TAU)
    C = [pt(p) for p in GF.G1.gen_muls(lcs)]
    W = pt(GF.G1.gen_muls([lw])[0])
    out = []
    oys, ows = k.open_fold(groups([polys]), scalars([z]), scalars([gamma]))
    ocs = k.commit(T.rows(polys))
    out.append(("made by open_fold and commit", [bytes(c) for c in ocs], z, gamma, [int.from_bytes(bytes(y), "little") for y in oys[0]], bytes(ows[0]), V))
    out.append(("made from tau alone", C, z, gamma, ys, W, V))
    out.append(("all-zero polynomials with W = O", [bytes(64)] * K, z, gamma, [0] * K, bytes(64), V))
    consts = [rnd.randrange(1, R) for _ in range(K)]
    Cc = [pt(p) for p in GF.G1.gen_muls(consts)]
    out.append(("constant polynomials", Cc, z, gamma, consts, bytes(64), V))
    _, yt, lwt = FM.logs(polys, TAU, gamma, TAU)
    out.append(("z = tau", C, TAU, gamma, yt, pt(GF.G1.gen_muls([lwt])[0]), V))
    _, y0, lw0 = FM.logs(polys, z, 0, TAU)
    out.append(("gamma = 0 is the first polynomial's opening", C, z, 0, y0, pt(GF.G1.gen_muls([lw0])[0]), V))
    out.append(("gamma = 0 does not bind the last value", C, z, 0, y0[:-1] + [(y0[-1] + 1) % R], pt(GF.G1.gen_muls([lw0])[0]), V))
    out.append(("the last y + 1", C, z, gamma, ys[:-1] + [(ys[-1] + 1) % R], W, E))
    out.append(("the first y + 1", C, z, gamma, [(ys[0] + 1) % R] + ys[1:], W, E))
    out.append(("2 C_1", [C[0], pt(GF.G1.gen_muls([2 * lcs[1]])[0])] + C[2:], z, gamma, ys, W, E))
    out.append(("gamma + 1", C, z, (gamma + 1) % R, ys, W, E))
    out.append(("z + 1", C, (z + 1) % R, gamma, ys, W, E))
    out.append(("a W with log q(tau) + 1", C, z, gamma, ys, pt(GF.G1.gen_muls([lw + 1])[0]), E))
    out.append(("constant polynomials with a wrong y", Cc, z, gamma, consts[:-1] + [(consts[-1] + 1) % R], bytes(64), E))
    out.append(("W at infinity for an f that is not constant", C, z, gamma, ys, bytes(64), E))
    out.append(("the last y = r", C, z, gamma, ys[:-1] + [R], W, S))
    out.append(("the first y = r", C, z, gamma, [R] + ys[1:], W, S))
    out.append(("gamma = r", C, z, R, ys, W, S))
    out.append(("z = r", C, R, gamma, ys, W, S))
    off = lambda c: c[:32] + ((int.from_bytes(c[32:], "little") + 1) % Q).to_bytes(32, "little")  # noqa: E731
    out.append(("the first C off the curve", [off(C[0])] + C[1:], z, gamma, ys, W, P))
    out.append(("the last C off the curve", C[:-1] + [off(C[-1])], z, gamma, ys, W, P))
    out.append(("a coordinate equal to q", C[:-1] + [Q.to_bytes(32, "little") + C[-1][32:]], z, gamma, ys, W, P))
    out.append(("a W off the curve", C, z, gamma, ys, W[:32] + bytes(31) + b"\x01", P))
    out.append(("y = r and a C off the curve: the scalar rule is first", [off(C[0])] + C[1:], z, gamma, ys[:-1] + [R], W, S))
    out.append(("gamma = r and a W off the curve: the scalar rule is first", C, z, R, ys, off(W), S))
    out.append(("a C off the curve and a wrong y: the point rule is first", C[:-1] + [off(C[-1])], z, gamma, [(ys[0] + 1) % R] + ys[1:], W, P))
    return out


def arrays(gs):
    c = np.frombuffer(b"".join(b"".join(g[1]) for g in gs), dtype=np.uint8).reshape(len(gs), -1, 64).copy()
    w = np.frombuffer(b"".join(g[5] for g in gs), dtype=np.uint8).reshape(-1, 64).copy()
    return c, scalars([g[2] for g in gs]), scalars([g[3] for g in gs]), values([g[4] for g in gs]), w


@pytest.mark.parametrize("power", POWERS)
def test_every_group_kind_in_one_mixed_batch(power):
    gs = mixed_groups(power)
    before = single_row_times(kzg(power), verify=False)
    got = kzg(power).verify_fold(*arrays(gs))
    assert got.dtype == np.uint32 and {g[0]: int(s) for g, s in zip(gs, got)} == {g[0]: g[6] for g in gs}
    ph = PKG.kzg_fold_phase_ms(kzg(power))
    assert ph["prepare"] > 0 and ph["pairing"] > 0 and ph["fold"] == ph["evals"] == ph["quotient"] == ph["lincomb"] == 0
    assert before["quotient"] > 0 and same_times(kzg(power), before)


def test_one_commitment_per_group_is_verify():
    rnd = random.Random(61)
    c, z, gamma, y, w = honest(rnd, 6, 1)
    bump(y, (1, 0))
    bump(z, 2)
    y[3, 0] = scalars([R])[0]
    w[4, 32] ^= 1
    got = kzg(4).verify_fold(c, z, gamma, y, w)
    assert list(got) == [V, E, E, S, P, V] == list(kzg(4).verify(c.reshape(6, 64), z, y.reshape(6, 32), w))


@pytest.mark.parametrize("K", (61, 62, 63, 65))
def test_a_wrong_last_value_past_the_first_chunk(K):
    """K + 2 terms: 63 are one below a chunk of the point fold, 64 fill it, 65 and 67 reach into a second; the wrong value is the last one"""
    rnd = random.Random(K)
    c, z, gamma, y, w = honest(rnd, 3, K, n=4)
    bump(y, (1, K - 1))
    y[2, K - 1] = scalars([R])[0]
    assert list(kzg(4).verify_fold(c, z, gamma, y, w)) == [V, E, S]
    c[0, K - 1, 0] ^= 1
    assert list(kzg(4).verify_fold(c, z, gamma, y, w)) == [P, E, S]


@pytest.mark.parametrize("count", (65, 257))
def test_one_bad_group_at_the_end_of_a_batch(count):
    rnd = random.Random(count)
    c, z, gamma, y, w = honest(rnd, count, 2)
    bump(y, (count - 1, 1))
    assert list(kzg(4).verify_fold(c, z, gamma, y, w)) == [V] * (count - 1) + [E]


# -- the twins, sub-batches, the CLI ------------------------------------------------------------------------------------------------
def test_host_and_device_twins_agree():
    import torch
    rnd = random.Random(71)
    k = kzg(4)
    polys = groups(random_groups(rnd, 3, 4, 16))
    zs, gammas = scalars([rnd.randrange(R) for _ in range(3)]), scalars([rnd.randrange(R) for _ in range(3)])
    cs = k.commit(polys.reshape(12, 16, 32)).reshape(3, 4, 64)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    d_z, d_g = cuda(zs), cuda(gammas)
    d_ys, d_ws = k.open_fold_device(cuda(polys), d_z, d_g, stream=s)
    d_st = k.verify_fold_device(cuda(cs), d_z, d_g, d_ys, d_ws, stream=s)
    d_bad = k.verify_fold_device(cuda(np.roll(cs, 1, axis=0)), d_z, d_g, d_ys, d_ws, stream=s)  # (one stream: the handle's workspace is one)
    s.synchronize()
    torch.cuda.synchronize()
    ys, ws = k.open_fold(polys, zs, gammas)
    assert np.array_equal(d_ys.cpu().numpy(), ys) and np.array_equal(d_ws.cpu().numpy(), ws)
    assert d_st.dtype == torch.int32 and list(d_st.cpu().numpy()) == [V] * 3 == list(k.verify_fold(cs, zs, gammas, ys, ws))
    assert list(d_bad.cpu().numpy()) == [E] * 3 == list(k.verify_fold(np.roll(cs, 1, axis=0), zs, gammas, ys, ws))


CHILD = """
import sys
import numpy as np
import cwc_import
pkg = cwc_import.load()
k = pkg.Kzg(open(sys.argv[1], "rb").read())
a = np.load(sys.argv[2])
ys, ws = k.open_fold(a["polys"], a["zs"], a["gammas"])
st = k.verify_fold(a["c"], a["vz"], a["vg"], a["vy"], a["vw"])
np.savez(sys.argv[3], ys=ys, ws=ws, st=st)
"""


def test_sub_batches_under_a_small_workspace_cap(tmp_path):
    """CWC_GROTH16_WORKSPACE_MB is read once per process, so a child process runs under 1 MB: 20 groups of 4 polynomials of 1 023
    coefficients (32 KB of folded polynomial and 32 KB of quotient each) are two sub-batches, and 257 checked groups (8.8 KB each
    with their pairings' workspace) are three.  The results are those of this process, whose cap is the default."""
    rnd = random.Random(81)
    polys = groups(random_groups(rnd, 20, 4, 1023))
    zs, gammas = scalars([rnd.randrange(R) for _ in range(20)]), scalars([rnd.randrange(R) for _ in range(20)])
    c, vz, vg, vy, vw = honest(rnd, 257, 2)
    bump(vy, (100, 1))
    (tmp_path / "pot.ptau").write_bytes(ptau(9))
    np.savez(tmp_path / "in.npz", polys=polys, zs=zs, gammas=gammas, c=c, vz=vz, vg=vg, vy=vy, vw=vw)
    env = dict(os.environ, CWC_GROTH16_WORKSPACE_MB="1")
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "pot.ptau"), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env, cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.load(tmp_path / "out.npz")
    ys, ws = kzg(9).open_fold(polys, zs, gammas)
    assert np.array_equal(got["ys"], ys) and np.array_equal(got["ws"], ws)
    assert list(got["st"]) == [E if i == 100 else V for i in range(257)] == list(kzg(9).verify_fold(c, vz, vg, vy, vw))


def test_the_cli_round_trip(tmp_path):
    rnd = random.Random(91)
    pot, z, gamma, ys, w, cs = (tmp_path / n for n in ("pot.ptau", "z.bin", "gamma.bin", "ys.bin", "w.bin", "cs.bin"))
    pot.write_bytes(ptau(4))
    polys = random_groups(rnd, 1, 3, 20)[0]
    zz, gg = rnd.randrange(R), rnd.randrange(R)
    z.write_bytes(zz.to_bytes(32, "little"))
    gamma.write_bytes(gg.to_bytes(32, "little"))
    run = lambda *a: subprocess.run([CLI] + [str(x) for x in a], capture_output=True, text=True)  # noqa: E731
    files = []
    for i, p in enumerate(polys):
        files.append(tmp_path / ("p%d.bin" % i))
        files[-1].write_bytes(bytes(le(p)))
        r = run("commit", pot, files[-1], tmp_path / ("c%d.bin" % i))
        assert r.returncode == 0, r.stderr
    cs.write_bytes(b"".join((tmp_path / ("c%d.bin" % i)).read_bytes() for i in range(3)))
    r = run("open-fold", pot, z, gamma, ys, w, *files)
    assert r.returncode == 0, r.stderr
    lcs, want_ys, lw = FM.logs(polys, zz, gg, TAU)
    assert cs.read_bytes() == bytes(points(lcs).reshape(-1)) and ys.read_bytes() == bytes(le(want_ys)) and w.read_bytes() == bytes(points([lw])[0])
    r = run("verify-fold", pot, cs, z, gamma, ys, w)
    assert r.returncode == 0 and r.stdout.strip() == "OK!", (r.stdout, r.stderr)
    flipped = bytearray(ys.read_bytes())
    flipped[64] ^= 1
    ys.write_bytes(bytes(flipped))
    r = run("verify-fold", pot, cs, z, gamma, ys, w)
    assert r.returncode == 1 and r.stdout.strip() == "EQUATION", (r.stdout, r.stderr)
