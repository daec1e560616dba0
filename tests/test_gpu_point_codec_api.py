"""The point codec through the library on an MI355X (r1cs/codec.hip, include/graph_witness_groth16_compressed.h), against the
plain-Python model of tests/point_codec_cases.py: gwb_bn254_compress_batch_device and gwb_bn254_decompress_batch_device for both
groups and both forms at n = 1, 63, 64, 65 and 129 with guard bytes behind every output (the C ABI is called directly, so that the
test owns the buffers), every refused encoding between lanes that decode, the argument errors, the Python wrappers, and the proof
kernels [B][256] <-> [B][128] at batches on both sides of a workgroup."""
import ctypes
import functools
import random

import numpy as np
import pytest

import cwc_import
from tests import point_codec_cases as PC

PKG = cwc_import.load()
pytestmark = pytest.mark.gpu
VALID, POINT = PKG.VERIFY_VALID, PKG.VERIFY_POINT
GUARD = 256
SIZES = (1, 63, 64, 65, 129)


def _cuda(b, width):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).reshape(-1, width).copy()).cuda()


def _guarded(nbytes):
    import torch
    return torch.full((nbytes + GUARD,), 0xa5, dtype=torch.uint8, device="cuda")


def _take(t, nbytes, what):
    """the first nbytes of a guarded buffer; the guard behind them must be untouched"""
    raw = t.cpu().numpy().tobytes()
    assert raw[nbytes:] == b"\xa5" * GUARD, what + ": bytes past the output were written"
    return raw[:nbytes]


def _call(fn, *args):
    import torch
    st = PKG.GwStatus()
    rc = fn(*args, torch.cuda.current_stream().cuda_stream, ctypes.byref(st))
    PKG._r1cs_check(rc, st)
    torch.cuda.synchronize()


def c_compress(group, form, points, n):
    d_in, out = _cuda(points, 64 * group), _guarded(32 * group * n)
    _call(PKG.r1cs_lib().gwb_bn254_compress_batch_device, d_in.data_ptr(), n, group, form, out.data_ptr())
    return _take(out, 32 * group * n, "compress")


def c_decompress(group, form, enc, n):
    d_in, out, status = _cuda(enc, 32 * group), _guarded(64 * group * n), _guarded(4 * n)
    _call(PKG.r1cs_lib().gwb_bn254_decompress_batch_device, d_in.data_ptr(), n, group, form, out.data_ptr(), status.data_ptr())
    return _take(out, 64 * group * n, "decompress"), list(np.frombuffer(_take(status, 4 * n, "decompress status"), dtype="<u4"))


@functools.lru_cache(maxsize=None)
def pool(group):
    """129 points (both signs of y by turns, infinity at every 7th place) -> (canonical bytes, Montgomery bytes, encodings): the
    model's reference, made once"""
    pts = PC.sample_points(group, 129)
    pb, comp = (PC.g1_bytes, PC.g1_compress) if group == 1 else (PC.g2_bytes, PC.g2_compress)
    larger = PC.fq_is_larger if group == 1 else PC.fq2_is_larger
    signs = {larger(p[1]) for p in pts if p is not None}
    assert signs == {True, False} and None in pts and pts[0] is not None
    return tuple(pb(p) for p in pts), tuple(pb(p, True) for p in pts), tuple(comp(p) for p in pts)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", (0, 1))
@pytest.mark.parametrize("group", (1, 2))
def test_round_trips_against_the_model(group, form, n):
    can, mont, enc = pool(group)
    first = 3 if n == 1 and form else 0   # the single point of one of the two n = 1 cases is infinity
    points = b"".join((mont if form else can)[first:first + n])
    want = b"".join(enc[first:first + n])
    assert c_compress(group, form, points, n) == want
    back, status = c_decompress(group, form, want, n)
    assert status == [VALID] * n and back == points
    assert c_compress(group, form, back, n) == want


@pytest.mark.parametrize("form", (0, 1))
@pytest.mark.parametrize("group", (1, 2))
def test_refused_encodings_between_lanes_that_decode(group, form):
    """every refused encoding at a lane of its own over three waves (lanes 0, 63, 64 among them), valid encodings around it: POINT and
    the point (0, 0) there, the neighbours' points as the model has them"""
    can, mont, enc = pool(group)
    bad = PC.refused_encodings(group, random.Random(31))
    n = 129
    at = [0, 63, 64, 128] + [k for k in range(2, 126, 5) if k not in (63, 64)]
    assert len(at) >= len(bad) and len(set(at)) == len(at)
    slots = dict(zip(at, bad))
    stream = b"".join(slots[i][1] if i in slots else enc[i] for i in range(n))
    back, status = c_decompress(group, form, stream, n)
    w = 64 * group
    for i in range(n):
        got = back[w * i:w * i + w]
        if i in slots:
            assert status[i] == POINT and got == bytes(w), "%s at lane %d" % (slots[i][0], i)
        else:
            assert status[i] == VALID and got == (mont if form else can)[i], "the valid encoding at lane %d" % i


def test_argument_errors_before_device_work():
    """an unknown group or form is refused with NULL buffers in hand: nothing can have been launched"""
    L = PKG.r1cs_lib()
    for fn, extra in ((L.gwb_bn254_compress_batch_device, ()), (L.gwb_bn254_decompress_batch_device, (None,))):
        for group, form, msg in ((3, 0, "group must be 1"), (0, 0, "group must be 1"), (1, 9, "form must be"), (2, 2, "form must be")):
            st = PKG.GwStatus()
            rc = fn(None, 5, group, form, None, *extra, None, ctypes.byref(st))
            assert rc == 1
            with pytest.raises(PKG.WitnessCalcError, match=msg):
                PKG._r1cs_check(rc, st)
        st = PKG.GwStatus()
        assert fn(None, 0, 1, 0, None, *extra, None, ctypes.byref(st)) == 0   # n = 0 does nothing


def test_python_wrappers():
    import torch
    for group, comp, dec in ((1, PKG.bn254_g1_compress_batch_device, PKG.bn254_g1_decompress_batch_device),
                             (2, PKG.bn254_g2_compress_batch_device, PKG.bn254_g2_decompress_batch_device)):
        can, mont, enc = pool(group)
        for form, src in ((False, can), (True, mont)):
            d = _cuda(b"".join(src[:70]), 64 * group)
            c = comp(d, montgomery=form)
            back, status = dec(c, montgomery=form)
            torch.cuda.synchronize()
            assert c.cpu().numpy().tobytes() == b"".join(enc[:70]) and torch.equal(back, d) and not status.any()
        empty = torch.empty((0, 64 * group), dtype=torch.uint8, device="cuda")
        assert tuple(comp(empty).shape) == (0, 32 * group)
        assert tuple(dec(torch.empty((0, 32 * group), dtype=torch.uint8, device="cuda"))[0].shape) == (0, 64 * group)


@pytest.mark.parametrize("batch", (1, 31, 32, 33, 64, 65))
def test_proof_kernels(batch):
    """[B][256] -> [B][128] equals the model row by row; back again with one refused point in some rows: POINT for the row, (0, 0) for
    that point, the row's other points decoded.  Batches on both sides of the G1 blocks' end (32 rows fill one) and of a G2 block."""
    g1c, _, g1e = pool(1)
    g2c, _, g2e = pool(2)
    rows = [g1c[(3 * i) % 129] + g2c[(5 * i + 1) % 129] + g1c[(3 * i + 2) % 129] for i in range(batch)]
    want = [g1e[(3 * i) % 129] + g2e[(5 * i + 1) % 129] + g1e[(3 * i + 2) % 129] for i in range(batch)]
    assert want == [PC.proof_compress(r) for r in rows]
    got = PKG.groth16_compress_proofs(np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(batch, 256))
    assert got.shape == (batch, 128) and got.tobytes() == b"".join(want)
    back, status = PKG.groth16_decompress_proofs(got)
    assert back.tobytes() == b"".join(rows) and list(status) == [VALID] * batch
    bad1, bad2 = PC.refused_encodings(1, random.Random(32)), PC.refused_encodings(2, random.Random(33))
    broken, expect, st = [], [], []
    for i in range(batch):
        c, r = bytearray(want[i]), bytearray(rows[i])
        which = (i + batch) % 4   # 0: A, 1: B, 2: C, 3: none
        if which == 0:
            c[:32], r[:64] = bad1[i % len(bad1)][1], bytes(64)
        elif which == 1:
            c[32:96], r[64:192] = bad2[i % len(bad2)][1], bytes(128)
        elif which == 2:
            c[96:], r[192:] = bad1[(i + 1) % len(bad1)][1], bytes(64)
        broken.append(bytes(c))
        expect.append(bytes(r))
        st.append(VALID if which == 3 else POINT)
    back, status = PKG.groth16_decompress_proofs(np.frombuffer(b"".join(broken), dtype=np.uint8).reshape(batch, 128))
    assert list(status) == st
    for i in range(batch):
        assert back[i].tobytes() == expect[i], "row %d" % i
