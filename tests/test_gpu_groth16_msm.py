"""The prover's multi-scalar multiplication (r1cs/msm.hip: digits_kernel, chunks_kernel, reduce_kernel, windows_kernel and the
assembly) on an MI355X at every window width c = 7 .. 15, on the scalar rows of tests/msm_fixtures.py, whose digit events and
chunk seams tests/test_msm_model_host.py counts on the host.

The oracle is exact: the keys are TiledKnownLog zkeys (every base has a known discrete log; P = 1031 distinct points per list,
tiled), used through Groth16(zkey) with no .r1cs, so a proof's three logs are dot products mod r and every comparison is byte
equality.  pi_A isolates MSM_A, pi_B isolates MSM_B2, pi_C carries B1, C and H.

Wire side: section 4 is the single entry (A, 0, 0, 1), so h = 0 for any witness and the H MSM adds nothing; nVars + 2 = 2^(c+3)
for c = 8 .. 15, and 2047 | 2048 and 262143 | 262144, the first and the last step of c.  One call per size, one row per class.
H side: A(x) = w_0 x, B(x) = w_0 x^(n-1) gives h_j = -2 w_0^2 at every point (r - 2 for w_0 = 1): domains 2^11 .. 2^18 drive the H
MSM at c = 8 .. 15 while the wire MSMs run at c = 7, the other order of the two shapes that share the workspace and the sentinel;
planted systems at 2^11 and 2^12 add uniform h scalars."""
import time

import numpy as np
import pytest

import cwc_import
from tests import msm_fixtures as MF
from tests import msm_model as M
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
R = F.R
PARTS = (("pi_A (MSM_A)", 0, 64), ("pi_B (MSM_B2)", 64, 192), ("pi_C (MSM_B1, MSM_C, MSM_H)", 192, 256))

pytestmark = pytest.mark.gpu


class Keys:
    """one key at a time: the handle of the previous size (its points and workspace on the device) is closed first"""

    def __init__(self):
        self.tag, self.key, self.g = None, None, None

    def get(self, tag, make):
        if self.tag != tag:
            self.close()
            t0 = time.time()
            self.key = make()
            self.g = PKG.Groth16(self.key.zkey)
            self.tag = tag
            print("key %s: %.1f s" % (tag, time.time() - t0))
        return self.key, self.g

    def close(self):
        if self.g is not None:
            self.g.close()
        self.tag, self.key, self.g = None, None, None


@pytest.fixture(scope="module")
def keys():
    k = Keys()
    yield k
    k.close()


def wire_key(keys, n_sc, inf=()):
    n_vars = n_sc - 2
    return keys.get(("wire", n_sc), lambda: MF.TiledKnownLog(n_vars, MF.N_PUB, 2, MF.ZERO_QUOTIENT, seed=n_sc, tweak=MF.wire_tweak(inf)))


def compare(got, want, names):
    bad = ["row %d (%s): %s" % (i, names[i], part) for i in range(len(names)) for part, lo, hi in PARTS
           if not np.array_equal(got[i, lo:hi], want[i, lo:hi])]
    assert not bad, "%d of %d proof parts differ: %s" % (len(bad), 3 * len(names), "; ".join(bad[:40]))


def want_of(key, rows, rs, h_logs=None):
    logs = [key.proof_logs(w, h_logs[i] if h_logs else 0, *rs[i]) for i, (_, w) in enumerate(rows)]
    return key.want_bytes(logs)


@pytest.mark.parametrize("n_sc", MF.WIRE_SIZES)
def test_wire_side_every_class(keys, n_sc):
    """uniform, digit edges, skew, bucket sweeps (windows 0 and n_win / 2, and r minus them), single buckets, cancellation and
    doubling on equal bases; infinity bases at c = 9 and 15; all ones at c = 8 and 15; (r, s) = (0, 0) on the rows built for
    one kind of digit or run, (r - 1, r - 1), (1, r - 1) and a random pair on the rows of random scalars (msm_fixtures.class_rs).
    At c = 10 also the rows as device rows above r and in Montgomery form."""
    shape, n_vars, inf, rows, rs = MF.wire_case(n_sc)
    key, g = wire_key(keys, n_sc, inf)
    names = [name for name, _ in rows]
    want = want_of(key, rows, rs)
    arr = F.rows_array([w for _, w in rows])
    compare(g.prove_batch(arr, rs=rs), want, names)
    if shape.c == 10:
        import torch
        pick = [names.index("uniform"), names.index("digit edges"), names.index("bucket sweep, window 0, negated")]
        sub = [rows[i][1] for i in pick]
        sub_rs, sub_want, sub_names = [rs[i] for i in pick], want[pick], [names[i] for i in pick]
        above = [[x + R if x + R < (1 << 256) and i % 3 == 1 else x for i, x in enumerate(w)] for w in sub]
        mont = [[F.to_montgomery(x) for x in w] for w in sub]
        mabove = [[x + R if x + R < (1 << 256) and i % 2 else x for i, x in enumerate(w)] for w in mont]
        assert any(x >= R for w in above for x in w) and any(x >= R for w in mabove for x in w)
        for form, montgomery in ((above, False), (mont, True), (mabove, True)):
            d = g.prove_batch_device(torch.from_numpy(F.rows_array(form)).cuda(), rs=sub_rs, montgomery=montgomery)
            torch.cuda.synchronize()
            compare(d.cpu().numpy(), sub_want, sub_names)


@pytest.mark.parametrize("n_sc", (2048, 16384))
def test_wire_side_batch_of_five(keys, n_sc):
    """the uniform and digit-edge classes as five rows of one call at c = 8 and 11: the key carries row n_win + window, and one
    sorted list holds every row"""
    shape = M.msm_shape(n_sc)
    key, g = wire_key(keys, n_sc)
    rows = MF.batch5_rows(shape, n_sc - 2, 7000 + n_sc)
    rs = MF.rs_pairs(5, 7 + n_sc)
    compare(g.prove_batch(F.rows_array([w for _, w in rows]), rs=rs), want_of(key, rows, rs), [name for name, _ in rows])


def h_tweak(p):
    inf = MF.h_infinity(p)
    return (lambda key: key.set_infinity("h", inf)) if inf else None


@pytest.mark.parametrize("p", MF.H_POWERS)
def test_h_side_constant_quotient(keys, p):
    """two rows with wire 0 = 1 and random other wires: every h scalar is r - 2, so each window of the H MSM has one bucket that
    holds all 2^p entries, and the H log is (r - 2) sum lh (H bases at infinity at 2^12 and 2^18 left out)"""
    n = 1 << p
    key, g = keys.get(("h", p), lambda: MF.TiledKnownLog(MF.H_N_VARS, MF.N_PUB, n, MF.constant_quotient(p), seed=p, tweak=h_tweak(p)))
    assert g.info["domain_size"] == n and M.msm_shape(n).c == p - 3 and M.msm_shape(MF.H_N_VARS + 2).c == 7
    rows = [("constant quotient", w) for w in MF.h_rows(p)]
    rs = MF.rs_pairs(5, p)[3:]
    h_log = key.dot("h", [R - 2] * n)
    compare(g.prove_batch(F.rows_array([w for _, w in rows]), rs=rs), want_of(key, rows, rs, [h_log] * 2), [name for name, _ in rows])


@pytest.mark.parametrize("p", MF.PLANTED_POWERS)
def test_h_side_planted_quotient(keys, p):
    """a planted system that fills the domain of 2^p (h from qap_reference.h_of, uniform below r) under a tiled key, three rows:
    the H MSM at c = 8 and 9 on random scalars"""
    n = 1 << p
    pl, ent, ws, hs = MF.planted_case(p)
    key, g = keys.get(("planted", p), lambda: MF.TiledKnownLog(pl.n_wires, MF.N_PUB, n, ent, seed=40 + p, tweak=h_tweak(p)))
    assert g.info["domain_size"] == n == g.qap_info()["domain_size"]
    rows = [("planted", w) for w in ws]
    rs = MF.rs_pairs(6, p)[3:]
    h_logs = [key.dot("h", h) for h in hs]
    compare(g.prove_batch(F.rows_array([w for _, w in rows]), rs=rs), want_of(key, rows, rs, h_logs), [name for name, _ in rows])
