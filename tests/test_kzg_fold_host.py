"""What the folded KZG openings (include/graph_witness_kzg.h, r1cs/kzg.cc) offer and refuse before they touch a device, through the
real library, on the files of tests/ptau_fixtures.py as tests/test_kzg_host.py uses them: the new names, a group of no
polynomials, a polynomial longer than the handle, arrays of the wrong shape, empty batches, and the kzg CLI's open-fold and
verify-fold usage, file and size errors (exit status 2).  All of this holds on a machine without a GPU."""
import functools
import os
import subprocess

import numpy as np
import pytest

import cwc_import
from tests import ptau_fixtures as PF

PKG = cwc_import.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "circom-witnesscalc_amd", "kzg")
TAU, ALPHA, BETA = 0x1234567, 0x89abcd, 0xfedcba9
POWER = 2
POINTS = (2 << POWER) - 1


@functools.lru_cache(maxsize=None)
def ptau():
    return PF.assemble(PF.sections(POWER, TAU, ALPHA, BETA, prepared=False))


def u8(*shape):
    return np.zeros(shape, dtype=np.uint8)


def refuses(pattern, call, *args, **kw):
    with pytest.raises(PKG.WitnessCalcError, match=pattern):
        call(*args, **kw)


def test_the_new_names():
    assert PKG.KZG_FOLD_PHASES == ("fold", "evals", "quotient", "lincomb", "prepare", "pairing")
    assert PKG.KZG_PHASES == ("quotient", "lincomb", "prepare", "pairing")
    for name in ("open_fold", "open_fold_device", "verify_fold", "verify_fold_device"):
        assert callable(getattr(PKG.Kzg, name)), name
    for name in ("kzg_fold_device", "kzg_fold_points_device", "kzg_fold_phase_ms"):
        assert callable(getattr(PKG, name)), name
    lib = PKG.r1cs_lib()
    for sym in ("gwb_kzg_open_fold_batch", "gwb_kzg_open_fold_batch_device", "gwb_kzg_verify_fold_batch", "gwb_kzg_verify_fold_batch_device",
                "gwb_kzg_fold_device", "gwb_kzg_fold_points_device", "gwb_kzg_fold_phase_ms"):
        assert getattr(lib, sym) is not None, sym


def test_a_group_of_no_polynomials_is_refused():
    k = PKG.Kzg(ptau())
    pattern = r"^kzg: a group of 0 polynomials$"
    refuses(pattern, k.open_fold, u8(2, 0, 4, 32), u8(2, 32), u8(2, 32))
    refuses(pattern, k.verify_fold, u8(2, 0, 64), u8(2, 32), u8(2, 32), u8(2, 0, 32), u8(2, 64))
    refuses(pattern, k.open_fold, u8(0, 0, 4, 32), u8(0, 32), u8(0, 32))  # also with no group at all


def test_more_pairs_than_the_kernels_index_are_refused():
    """G K above 2^31 - 1, through the raw ABI: the refusal comes before an address is looked at, so small buffers stand in"""
    lib, call = PKG.r1cs_lib(), PKG._r1cs_call
    buf = u8(64)
    a = buf.ctypes.data
    k = PKG.Kzg(ptau())
    for g, n in ((1 << 31, 1), (1 << 16, 1 << 15), (1 << 40, 1 << 40)):
        pattern = r"^kzg: %d groups of %d are more than 2\^31 - 1 \(polynomial, point\) pairs$" % (g, n)
        refuses(pattern, call, lib.gwb_kzg_fold_device, a, a, g, n, 1, a, None)
        refuses(pattern, call, lib.gwb_kzg_fold_points_device, a, a, g, n, a, None)
        refuses(pattern, call, lib.gwb_kzg_open_fold_batch, k._h, a, a, a, g, n, 1, a, a)
        refuses(pattern, call, lib.gwb_kzg_open_fold_batch_device, k._h, a, a, a, g, n, 1, a, a, None)
        refuses(pattern, call, lib.gwb_kzg_verify_fold_batch, k._h, a, a, a, a, a, g, n, a)
        refuses(pattern, call, lib.gwb_kzg_verify_fold_batch_device, k._h, a, a, a, a, a, g, n, a, None)
    call(lib.gwb_kzg_fold_device, a, a, (1 << 31) - 1, 1, 0, a, None)  # at the limit, and N = 0: nothing to do


def test_a_polynomial_longer_than_the_handle_is_refused():
    k = PKG.Kzg(ptau(), max_len=5)
    refuses(r"^kzg: a polynomial of 6 coefficients is above the handle's max_len 5$", k.open_fold, u8(2, 3, 6, 32), u8(2, 32), u8(2, 32))


def test_empty_batches_return_without_a_device():
    k = PKG.Kzg(ptau())
    ys, ws = k.open_fold(u8(0, 3, 4, 32), u8(0, 32), u8(0, 32))
    assert ys.shape == (0, 3, 32) and ys.dtype == np.uint8 and ws.shape == (0, 64)
    st = k.verify_fold(u8(0, 3, 64), u8(0, 32), u8(0, 32), u8(0, 3, 32), u8(0, 64))
    assert st.shape == (0,) and st.dtype == np.uint32
    refuses(r"^no KZG fold phase times", PKG.kzg_fold_phase_ms, k)


def test_wrong_shapes_are_refused_in_python():
    k = PKG.Kzg(ptau())
    z = u8(2, 32)
    refuses(r"^kzg: polys: uint8 \[G, K, N, 32\] expected, got \[2, 4, 32\]$", k.open_fold, u8(2, 4, 32), z, z)
    refuses(r"^kzg: polys: uint8 \[G, K, N, 32\] expected, got \[2, 3, 4, 31\]$", k.open_fold, u8(2, 3, 4, 31), z, z)
    refuses(r"^kzg: zs: uint8 \[G, 32\] expected", k.open_fold, u8(2, 3, 4, 32), u8(2, 33), z)
    refuses(r"^kzg: gammas: uint8 \[G, 32\] expected", k.open_fold, u8(2, 3, 4, 32), z, u8(2, 1, 32))
    refuses(r"^kzg: 2 groups, 3 points and 2 challenges$", k.open_fold, u8(2, 3, 4, 32), u8(3, 32), z)
    refuses(r"^kzg: 2 groups, 2 points and 1 challenges$", k.open_fold, u8(2, 3, 4, 32), z, z[:1])
    c, y, w = u8(2, 3, 64), u8(2, 3, 32), u8(2, 64)
    refuses(r"^kzg: commitments: uint8 \[G, K, 64\] expected, got \[2, 64\]$", k.verify_fold, u8(2, 64), z, z, y, w)
    refuses(r"^kzg: ys: uint8 \[G, K, 32\] expected", k.verify_fold, c, z, z, z, w)
    refuses(r"^kzg: proofs: uint8 \[G, 64\] expected", k.verify_fold, c, z, z, y, u8(2, 65))
    refuses(r"^kzg: 2 groups of 3 commitments, 2 points, 2 challenges, 2 groups of 4 values and 2 proofs$", k.verify_fold, c, z, z, u8(2, 4, 32), w)
    refuses(r"^kzg: 2 groups of 3 commitments, 2 points, 1 challenges, 2 groups of 3 values and 2 proofs$", k.verify_fold, c, z, z[:1], y, w)
    refuses(r"^kzg: d_polys: a contiguous uint8 cuda tensor \[G, K, N, 32\] expected$", k.open_fold_device, u8(2, 3, 4, 32), z, z)
    refuses(r"^kzg: d_commitments: a contiguous uint8 cuda tensor \[G, K, 64\] expected$", k.verify_fold_device, c, z, z, y, w)
    refuses(r"^kzg: d_polys: a contiguous uint8 cuda tensor", PKG.kzg_fold_device, u8(2, 3, 4, 32), z)
    refuses(r"^kzg: d_points: a contiguous uint8 cuda tensor", PKG.kzg_fold_points_device, c, z)


def run_cli(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True)


def test_the_cli_parses_its_inputs_before_the_device(tmp_path):
    pot, p0, p1, z, cs, out = (tmp_path / n for n in ("pot.ptau", "p0.bin", "p1.bin", "z.bin", "cs.bin", "out.bin"))
    pot.write_bytes(ptau())
    p0.write_bytes(bytes(32 * 3))
    p1.write_bytes(bytes(32 * 2))
    z.write_bytes(bytes(32))
    cs.write_bytes(bytes(64 * 2))
    for args in (("open-fold", pot, z, z, out, out), ("open-fold",), ("verify-fold", pot, cs, z, z, z), ("verify-fold", pot, cs, z, z, z, cs, cs)):
        r = run_cli(*args)
        assert r.returncode == 2 and "kzg open-fold <pot.ptau> <z.bin> <gamma.bin> <ys.bin> <proof.bin> <poly0.bin> [<poly1.bin> ...]" in r.stderr, args
        assert "kzg verify-fold <pot.ptau> <commitments.bin> <z.bin> <gamma.bin> <ys.bin> <proof.bin>" in r.stderr
    r = run_cli("open-fold", pot, z, z, out, out, p0, p1)
    assert r.returncode == 2 and "64 bytes" in r.stderr and "has 96: the polynomials of a group have one length" in r.stderr
    r = run_cli("open-fold", pot, z, z, out, out, p0, tmp_path / "absent.bin")
    assert r.returncode == 2 and "cannot read" in r.stderr
    p1.write_bytes(bytes(33))
    r = run_cli("open-fold", pot, z, z, out, out, p0, p1)
    assert r.returncode == 2 and "33 bytes, a polynomial is a positive number of 32-byte coefficients" in r.stderr
    p1.write_bytes(bytes(31))
    r = run_cli("open-fold", pot, z, p1, out, out, p0)
    assert r.returncode == 2 and "31 bytes, a scalar is 32" in r.stderr
    p0.write_bytes(bytes(32 * (POINTS + 1)))
    r = run_cli("open-fold", pot, z, z, out, out, p0, p0)
    assert r.returncode == 2 and "kzg: max_len %d is above" % (POINTS + 1) in r.stderr
    # verify-fold: two commitments want 64 bytes of values
    r = run_cli("verify-fold", pot, cs, z, z, z, cs)
    assert r.returncode == 2 and "32 bytes, a value per commitment is 64" in r.stderr
    r = run_cli("verify-fold", pot, p1, z, z, z, cs)
    assert r.returncode == 2 and "31 bytes, the commitments are a positive number of 64-byte points" in r.stderr
    ys = tmp_path / "ys.bin"
    ys.write_bytes(bytes(64))
    r = run_cli("verify-fold", pot, cs, z, z, ys, cs)
    assert r.returncode == 2 and "128 bytes, a proof is 64" in r.stderr
    pot.write_bytes(ptau()[:100])
    r = run_cli("verify-fold", pot, cs, z, z, ys, z.parent / "cs1.bin")
    assert r.returncode == 2 and "cannot read" in r.stderr
    (tmp_path / "cs1.bin").write_bytes(bytes(64))
    r = run_cli("verify-fold", pot, cs, z, z, ys, tmp_path / "cs1.bin")
    assert r.returncode == 2 and "error: ptau: " in r.stderr
    assert not out.exists()
