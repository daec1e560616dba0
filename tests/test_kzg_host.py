"""What the KZG layer (include/graph_witness_kzg.h, r1cs/kzg.cc) refuses before it touches a device, through the real library, on
files written by tests/ptau_fixtures.py: a handle's max_len and file, a polynomial longer than the handle, commit_evals on a file
that is not prepared or for more evaluations than the handle covers, buffers of the wrong shape, and the kzg CLI's usage, file
and format errors (exit status 2).  Making a handle without check_powers reads and checks the file's points on the host only, so
all of this holds on a machine without a GPU."""
import functools
import os
import subprocess

import numpy as np
import pytest

import cwc_import
from tests import groth16_fixtures as GF
from tests import ptau_fixtures as PF

PKG = cwc_import.load()
R, Q = GF.R, GF.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "circom-witnesscalc_amd", "kzg")
TAU, ALPHA, BETA = 0x1234567, 0x89abcd, 0xfedcba9
POWER = 2
POINTS = (2 << POWER) - 1


@functools.lru_cache(maxsize=None)
def secs(prepared=False):
    return PF.sections(POWER, TAU, ALPHA, BETA, prepared=prepared)


@functools.lru_cache(maxsize=None)
def ptau(prepared=False):
    return PF.assemble(secs(prepared))


def polys(k, n):
    return np.zeros((k, n, 32), dtype=np.uint8)


def refuses(pattern, call, *args, **kw):
    with pytest.raises(PKG.WitnessCalcError, match=pattern):
        call(*args, **kw)


def test_the_tiles():
    tiles = PKG.kzg_tiles()
    assert tiles[0] == 256 and len(tiles) >= 2 and tiles == sorted(set(tiles)) and all(t % 256 == 0 for t in tiles)


def test_the_statuses():
    assert (PKG.KZG_VALID, PKG.KZG_SCALAR, PKG.KZG_POINT, PKG.KZG_EQUATION) == (0, 1, 2, 3)


def test_a_handle_and_its_info():
    k = PKG.Kzg(ptau())
    assert k.info == {"max_len": POINTS, "power": POWER, "prepared": False}
    assert PKG.Kzg(ptau(True), max_len=3).info == {"max_len": 3, "power": POWER, "prepared": True}
    k.close()
    k.close()


def test_max_len_is_refused():
    refuses(r"^kzg: max_len is 0$", PKG.Kzg, ptau(), max_len=0)
    refuses(r"^kzg: max_len %d is above the 2\^\(power\+1\) - 1 = %d points" % (POINTS + 1, POINTS), PKG.Kzg, ptau(), max_len=POINTS + 1)
    PKG.Kzg(ptau(), max_len=POINTS)


def test_a_malformed_file_is_refused():
    data = ptau()
    refuses(r"^ptau: ", PKG.Kzg, data[:len(data) - 7])
    refuses(r"^ptau: ", PKG.Kzg, data[:40])
    refuses(r"^ptau: ", PKG.Kzg, b"")
    refuses(r"^ptau: ", PKG.Kzg, b"ptbu" + data[4:])


def test_a_wrong_point_is_refused_with_its_index():
    s = dict(secs())
    off = 3 * 64 + 32  # the y of tauG1[3]
    s[2] = s[2][:off] + GF.lem(1) + s[2][off + 32:]
    bad = PF.assemble(s)
    refuses(r"^ptau: section 2 \(tauG1\) point 3 is not on the G1 curve$", PKG.Kzg, bad)
    PKG.Kzg(bad, max_len=3)  # the handle reads the prefix it covers and no more
    s = dict(secs())
    s[3] = s[3][:128] + (Q).to_bytes(32, "little") + s[3][160:]
    refuses(r"^ptau: section 3 \(tauG2\) point 1 has a coordinate >= q$", PKG.Kzg, PF.assemble(s), max_len=1)


def test_a_polynomial_longer_than_the_handle_is_refused():
    k = PKG.Kzg(ptau(), max_len=5)
    z = np.zeros((2, 32), dtype=np.uint8)
    pattern = r"^kzg: a polynomial of 6 coefficients is above the handle's max_len 5$"
    refuses(pattern, k.commit, polys(2, 6))
    refuses(pattern, k.open, polys(2, 6), z)


def test_commit_evals_needs_a_prepared_file_and_a_covered_level():
    refuses(r"^ptau: lagrange = file, but the file has no prepared sections 12 to 15", PKG.Kzg(ptau()).commit_evals, polys(1, 4))
    k = PKG.Kzg(ptau(True), max_len=5)
    refuses(r"^kzg: 2\^3 evaluations are above the handle's max_len 5$", k.commit_evals, polys(1, 8))
    refuses(r"^kzg: evals: 3 evaluations, a power of two expected$", k.commit_evals, polys(1, 3))


def test_empty_batches_return_without_a_device():
    k = PKG.Kzg(ptau())
    assert k.commit(polys(0, 4)).shape == (0, 64)
    ys, ws = k.open(polys(0, 4), np.zeros((0, 32), dtype=np.uint8))
    assert ys.shape == (0, 32) and ws.shape == (0, 64)
    assert k.verify(np.zeros((0, 64), np.uint8), np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8), np.zeros((0, 64), np.uint8)).shape == (0,)


def test_wrong_shapes_are_refused_in_python():
    k = PKG.Kzg(ptau())
    z = np.zeros((2, 32), dtype=np.uint8)
    refuses(r"^kzg: polys: uint8 \[K, N, 32\] expected, got \[2, 4, 31\]$", k.commit, np.zeros((2, 4, 31), dtype=np.uint8))
    refuses(r"^kzg: polys: uint8 \[K, N, 32\] expected", k.commit, np.zeros((4, 32), dtype=np.uint8))
    refuses(r"^kzg: zs: uint8 \[K, 32\] expected", k.open, polys(2, 4), np.zeros((2, 33), dtype=np.uint8))
    refuses(r"^kzg: 2 polynomials and 3 points$", k.open, polys(2, 4), np.zeros((3, 32), dtype=np.uint8))
    refuses(r"^kzg: 2 polynomials and 3 points$", k.eval, polys(2, 4), np.zeros((3, 32), dtype=np.uint8))
    c, w = np.zeros((2, 64), dtype=np.uint8), np.zeros((2, 64), dtype=np.uint8)
    refuses(r"^kzg: commitments: uint8 \[K, 64\] expected", k.verify, np.zeros((2, 32), dtype=np.uint8), z, z, w)
    refuses(r"^kzg: proofs: uint8 \[K, 64\] expected", k.verify, c, z, z, np.zeros((2, 65), dtype=np.uint8))
    refuses(r"^kzg: 2 commitments, 2 points, 1 values and 2 proofs$", k.verify, c, z, z[:1], w)
    refuses(r"^kzg: d_polys: a contiguous uint8 cuda tensor", k.commit_device, polys(2, 4))
    refuses(r"^kzg: d_polys: a contiguous uint8 cuda tensor", PKG.kzg_eval_quotient_device, polys(2, 4), z)
    refuses(r"^no KZG phase times", PKG.kzg_phase_ms, k)


def run_cli(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True)


def test_the_cli_parses_its_inputs_before_the_device(tmp_path):
    pot, poly, z, out = (tmp_path / n for n in ("pot.ptau", "poly.bin", "z.bin", "out.bin"))
    pot.write_bytes(ptau())
    poly.write_bytes(bytes(32 * 3))
    z.write_bytes(bytes(32))
    for args in ((), ("commit", pot, poly), ("open", pot, poly, z, out), ("verify", pot, out, z, z), ("prove", pot, poly, out)):
        r = run_cli(*args)
        assert r.returncode == 2 and "usage: kzg commit" in r.stderr, args
    r = run_cli("commit", tmp_path / "absent.ptau", poly, out)
    assert r.returncode == 2 and "cannot read" in r.stderr
    r = run_cli("commit", pot, tmp_path / "absent.bin", out)
    assert r.returncode == 2 and "cannot read" in r.stderr
    poly.write_bytes(bytes(33))
    r = run_cli("commit", pot, poly, out)
    assert r.returncode == 2 and "33 bytes, a polynomial is a positive number of 32-byte coefficients" in r.stderr
    poly.write_bytes(bytes(32 * (POINTS + 1)))
    r = run_cli("commit", pot, poly, out)
    assert r.returncode == 2 and "kzg: max_len %d is above" % (POINTS + 1) in r.stderr
    z.write_bytes(bytes(31))
    poly.write_bytes(bytes(64))
    r = run_cli("open", pot, poly, z, out, out)
    assert r.returncode == 2 and "31 bytes, a scalar is 32" in r.stderr
    r = run_cli("verify", pot, poly, z, z, poly)
    assert r.returncode == 2 and "31 bytes, a scalar is 32" in r.stderr
    pot.write_bytes(ptau()[:100])
    z.write_bytes(bytes(32))
    r = run_cli("verify", pot, poly, z, z, poly)
    assert r.returncode == 2 and "error: ptau: " in r.stderr
    assert not out.exists()
