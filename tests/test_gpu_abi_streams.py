"""The skeleton of the package's asynchronous device calls (_device_call in circom-witnesscalc_amd/__init__.py) on an MI355X, at
the smallest sizes: a call on a side stream while the default stream is current gives what the call on the current stream gives,
and an empty batch is no error."""
import numpy as np
import pytest

import cwc_import
from tests import bn254_pairing as BP
from tests import groth16_fixtures as GF
from tests import r1cs_fixtures as RF

pytestmark = pytest.mark.gpu
PKG = cwc_import.load()
SCALARS = (1, 2, GF.R - 1)


def host_multiple(k):
    """k times the generator of G1 by double-and-add over tests/bn254_pairing.py's curve arithmetic, as 64 canonical bytes"""
    base, acc = (BP.f12(GF.G1_GEN[0]), BP.f12(GF.G1_GEN[1])), None
    while k:
        if k & 1:
            acc = BP._add(acc, base)
        base, k = BP._double(base), k >> 1
    assert not any(acc[0][1:]) and not any(acc[1][1:])
    return acc[0][0].to_bytes(32, "little") + acc[1][0].to_bytes(32, "little")


def test_gen_mul_on_a_side_stream():
    import torch
    d_k = torch.from_numpy(np.frombuffer(b"".join(k.to_bytes(32, "little") for k in SCALARS), dtype=np.uint8).reshape(3, 32).copy()).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert torch.cuda.current_stream() != side
    on_side = PKG.bn254_gen_mul_batch_device(d_k, 1, stream=side)
    side.synchronize()
    got = on_side.cpu().numpy().tobytes()
    on_current = PKG.bn254_gen_mul_batch_device(d_k, 1)
    torch.cuda.synchronize()
    assert tuple(on_side.shape) == (3, 64) and got == on_current.cpu().numpy().tobytes()
    assert got == b"".join(host_multiple(k) for k in SCALARS)


def test_gen_mul_of_no_scalars():
    import torch
    out = PKG.bn254_gen_mul_batch_device(torch.empty((0, 32), dtype=torch.uint8, device="cuda"), 1, stream=torch.cuda.Stream())
    torch.cuda.synchronize()
    assert tuple(out.shape) == (0, 64)


def test_r1cs_check_on_a_side_stream():
    import torch
    constraints = [({1: 1}, {2: 1}, {3: 1}), ({1: 1}, {1: 1}, {2: 1})]  # w1 w2 = w3 and w1^2 = w2
    rows = [[1, 3, 9, 27], [1, 3, 9, 28]]
    r = PKG.R1cs(RF.write_r1cs(4, constraints))
    d_w = torch.from_numpy(RF.rows_array(rows)).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    first_s, nfail_s = r.check_batch_device(d_w, stream=side)
    side.synchronize()
    first, nfail = r.check_batch_device(d_w)
    torch.cuda.synchronize()
    for t in (first_s, nfail_s, first, nfail):
        assert t.dtype == torch.int32 and tuple(t.shape) == (2,)
    assert torch.equal(first_s, first) and torch.equal(nfail_s, nfail)
    want = [RF.check(constraints, w) for w in rows]
    assert first.cpu().numpy().astype(np.uint32).tolist() == [f for f, _ in want] == [PKG.R1CS_SATISFIED, 0]
    assert nfail.tolist() == [n for _, n in want] == [0, 1]
