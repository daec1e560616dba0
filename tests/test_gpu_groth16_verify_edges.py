"""The Groth16 verifier and the pairing aid (r1cs/verify.hip) on an MI355X at their seams: batches that cross the 64-thread
workgroups of check_kernel, miller_kernel, easy_kernel, final_kernel and pairs_kernel (63, 64, 65, 130 rows: a second block, a
partial last block, the spill buffer's interleaved layout at rows >= 64, skipped rows beside working rows), one key's workspace
reused across batch sizes, vkx_kernel's groups of 8 signals (nPublic 7, 8, 9, 16, 17), the exceptional additions of vk_x driven
through the verifier by keys with chosen IC logs (a doubling and a cancellation inside a window, equal and opposite partial sums
across groups, IC points at infinity, vk_x = O), and degenerate keys (gamma2, delta2, alpha1, beta2 at infinity).

Every call goes through both entry points (host memory and device memory, which must agree).  Expected statuses come from the
logs alone: a b = alpha beta + gamma ic(pub) + delta c (mod r) decides VALID or EQUATION unless the row was tampered with
(PUBLIC, POINT, SUBGROUP); expected GT bytes are powers of one oracle pairing."""
import functools
import itertools
import random

import numpy as np
import pytest

from tests import bn254_pairing as BP
from tests import groth16_fixtures as GF
from tests import test_gpu_groth16_verify as V

pytestmark = pytest.mark.gpu
R, Q = GF.R, GF.Q
PKG, Key = V.PKG, V.Key
VALID, PUBLIC, POINT, SUBGROUP, EQUATION = V.VALID, V.PUBLIC, V.POINT, V.SUBGROUP, V.EQUATION
SEAM_BATCHES = (63, 64, 65, 130)
# the kinds of the singled-out rows (rows 0, 63, 64 and the last one, as far as a batch has them)
KINDS = ("PUBLIC", "A = O", "POINT", "B = O", "SUBGROUP", "C = O", "EQUATION")
STATUS = {"PUBLIC": PUBLIC, "POINT": POINT, "SUBGROUP": SUBGROUP, "EQUATION": EQUATION, "VALID": VALID, "A = O": VALID, "B = O": VALID,
          "C = O": VALID}


def seam_rows(batch):
    return sorted({r for r in (0, 63, 64, batch - 1) if r < batch})


@functools.lru_cache(maxsize=None)
def pairing_of_generators():
    return BP.pairing(GF.G1_GEN, GF.G2_GEN)


@functools.lru_cache(maxsize=None)
def outside_subgroup():
    return BP.twist_point_outside_subgroup(random.Random(5))


def inv(x):
    return pow(x, -1, R)


def make_rows(key, plan, pubs):
    """plan: one kind per row -> (proof rows, signals as given to the verifier, expected statuses from the logs and the tamper)"""
    rnd, logs = key.rnd, []
    for kind, pub in zip(plan, pubs):
        a, b = rnd.randrange(1, R), rnd.randrange(1, R)
        if kind == "A = O":
            a = 0
        if kind == "B = O":
            b = 0
        c = key.c_for(a, b, pub)
        if kind == "C = O":
            c, b = 0, (key.alpha * key.beta + key.gamma * key.ic_log(pub)) * inv(a) % R
        if kind == "EQUATION":
            c = (c + 1 + rnd.randrange(R - 1)) % R
        logs.append((a, b, c))
    assert len(set(logs)) == len(logs)   # a distinct proof per row
    rows = V._proof_rows(logs)
    pubs = [list(p) for p in pubs]
    want = []
    for i, (kind, (a, b, c)) in enumerate(zip(plan, logs)):
        st = VALID if key.holds(a, b, c, pubs[i]) else EQUATION   # (before the tamper: the signals still below r)
        if kind == "PUBLIC":
            pubs[i][-1] += R
            st = PUBLIC
        if kind == "POINT":   # A.y + 1: off the curve
            v = (int.from_bytes(bytes(rows[i, 32:64]), "little") + 1) % Q
            rows[i, 32:64] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
            st = POINT
        if kind == "SUBGROUP":
            rows[i, 64:192] = np.frombuffer(V._g2b(outside_subgroup()), np.uint8)
            st = SUBGROUP
        assert st == STATUS[kind], (i, kind)
        want.append(st)
    for kind, row in zip(plan, rows):
        assert (not row[:64].any()) == (kind == "A = O") and (not row[64:192].any()) == (kind == "B = O") and (not row[192:].any()) == (kind == "C = O")
    return rows, pubs, want


# Which singled-out rows are VALID.  Adjacent rows differ in status, so at most every other row is VALID: half of a batch can be
# VALID only if its singled-out rows fall in with one alternation.  The batch of 65 gives its last block (row 64 alone) to a row
# that is not VALID, which leaves it 32 VALID rows of 65, the most that allows; the others have at least half.
SEAM_VALID = {63: {0: True, 62: True}, 64: {0: True, 63: False}, 65: {0: True, 63: False, 64: False}, 130: {0: False, 63: True, 64: False, 129: True}}


def seam_plan(batch, valid_kinds, other_kinds):
    """the singled-out rows take the next kind of their list; every other row is VALID where its neighbours allow it, else
    EQUATION or POINT, so that adjacent rows differ in status"""
    plan = [None] * batch
    assert sorted(SEAM_VALID[batch]) == seam_rows(batch)
    for r in seam_rows(batch):
        plan[r] = next(valid_kinds if SEAM_VALID[batch][r] else other_kinds)
    for i in range(batch):
        if plan[i] is None:
            taken = {STATUS[plan[j]] for j in (i - 1, i + 1) if 0 <= j < batch and plan[j] is not None}
            plan[i] = next(k for k in ("VALID", "EQUATION", "POINT") if STATUS[k] not in taken)
    st = [STATUS[k] for k in plan]
    last_block = st[(batch - 1) // 64 * 64:]
    assert all(x != y for x, y in zip(st, st[1:]))
    assert 2 * st.count(VALID) >= batch or (VALID not in last_block and st.count(VALID) == batch // 2)
    return plan


@functools.lru_cache(maxsize=None)
def seam_plans():
    """the kinds rotate over the batches: the three VALID ones over the rows of SEAM_VALID that are VALID, the four others over
    the rest"""
    valid_kinds = itertools.cycle(k for k in KINDS if STATUS[k] == VALID)
    other_kinds = itertools.cycle(k for k in KINDS if STATUS[k] != VALID)
    plans = {batch: seam_plan(batch, valid_kinds, other_kinds) for batch in SEAM_BATCHES}
    on_seams = {plans[b][r] for b in SEAM_BATCHES for r in seam_rows(b)}
    assert on_seams == set(KINDS)   # each of the seven kinds lands on a singled-out row
    # one batch's last block holds only rows that are not VALID
    assert any(all(STATUS[k] != VALID for k in plans[b][(b - 1) // 64 * 64:]) for b in SEAM_BATCHES)
    return plans


# -- 1: batch seams -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", SEAM_BATCHES)
def test_batch_seams(batch):
    key = Key(2, 100 + batch)
    plan = seam_plans()[batch]
    rows, pubs, want = make_rows(key, plan, V._signals(key.rnd, 2, batch))
    assert list(V._verify_both(key, rows, pubs)) == want


# -- 2: the pairing aid's seams -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SEAM_BATCHES)
def test_pairing_aid_seams(n):
    rnd = random.Random(200 + n)
    ab = [[rnd.randrange(1, R), rnd.randrange(1, R)] for _ in range(n)]
    zero = ((True, False), (False, True), (True, True))   # (O, Q), (P, O), (O, O), one kind after another
    k = sum(len(seam_rows(m)) for m in SEAM_BATCHES if m < n)
    for j, r in enumerate(seam_rows(n)):
        za, zb = zero[(k + j) % 3]
        ab[r] = [0 if za else ab[r][0], 0 if zb else ab[r][1]]
    ps = GF.G1.gen_muls([a for a, _ in ab])
    qs = GF.G2.gen_muls([b for _, b in ab])
    assert all((p is None) == (a == 0) and (q is None) == (b == 0) for (a, b), p, q in zip(ab, ps, qs))
    got = V._pair_dev(ps, qs)
    e = pairing_of_generators()
    for i, ((a, b), g) in enumerate(zip(ab, got)):
        assert g == BP.gt_bytes(BP.power(e, a * b % R)), i
    for r in seam_rows(n):
        assert got[r] == BP.gt_bytes(BP.ONE)


# -- 3: one key's workspace across batch sizes --------------------------------------------------------------------------------------
def test_workspace_reuse_across_batch_sizes():
    key = Key(2, 300)
    ab = key.vk.alphabeta()
    assert ab == BP.gt_bytes(BP.power(pairing_of_generators(), key.alpha * key.beta % R))
    plan = ["VALID" if i % 3 != 1 else "EQUATION" for i in range(130)]
    rows, pubs, want = make_rows(key, plan, V._signals(key.rnd, 2, 130))
    results = []
    for lo, hi in ((0, 130), (7, 8), (65, 130), (63, 65), (0, 130)):   # 130, 1, 65, 2, 130 rows
        got = list(V._verify_both(key, rows[lo:hi].copy(), pubs[lo:hi]))
        assert got == want[lo:hi], (lo, hi)
        results.append(got)
    assert results[0] == results[-1]
    assert key.vk.alphabeta() == ab


# -- 4: vk_x's groups of eight signals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_public", [7, 8, 9, 16, 17])
def test_vkx_group_seams(n_public):
    key = Key(n_public, 400 + n_public)
    rnd = key.rnd
    edge = (1, 1 << 252, R - 1)   # the bottom window only, the top window only, the largest
    pubs = V._signals(rnd, n_public, 2)
    pubs += [[0] * (n_public - 1) + [s] for s in edge]
    if n_public > 8:
        pubs += [[s if i == 8 else 0 for i in range(n_public)] for s in edge]
    assert len(pubs) == (8 if n_public > 8 else 5)
    rows = V._proof_rows(key.forge(pubs))
    assert list(V._verify_both(key, rows, pubs)) == [VALID] * len(pubs)
    for i in (1, 3):   # a random row, and the row whose only signal is 2^252
        wrong = [list(p) for p in pubs]
        wrong[i][-1] = (wrong[i][-1] + 1) % R
        assert list(V._verify_both(key, rows, wrong)) == [VALID if j != i else EQUATION for j in range(len(pubs))]


# -- 5: vk_x's exceptional additions ---------------------------------------------------------------------------------------------------
def _vkx_cases():
    """name -> (chosen IC logs, signals): nPublic 9, so signals 1 .. 8 share vkx_kernel's first group and signal 9 has the second"""
    rnd = random.Random(500)
    u, s, t = (rnd.randrange(1, R) for _ in range(3))
    rest = [rnd.randrange(1, R) for _ in range(9)]
    only_1_and_9 = [s] + [0] * 7 + [s]
    ic0 = rnd.randrange(1, R)
    return {
        "IC_1 = IC_2, s_1 = s_2: a doubling inside a window": ({1: u, 2: u}, [s, s] + rest[2:]),
        "IC_2 = -IC_1, s_1 = s_2: back to infinity in every window": ({1: u, 2: -u}, [s, s] + rest[2:]),
        "IC_9 = IC_1, equal partial sums, IC_0 = O": ({0: 0, 1: u, 9: u}, only_1_and_9),
        "IC_9 = IC_1, equal partial sums": ({1: u, 9: u}, only_1_and_9),
        "IC_9 = -IC_1, opposite partial sums, vk_x = IC_0": ({1: u, 9: -u}, only_1_and_9),
        "IC_9 = -IC_1, opposite partial sums, IC_0 = O, vk_x = O": ({0: 0, 1: u, 9: -u}, only_1_and_9),
        "IC_3 = O under a nonzero signal": ({3: 0}, rest),
        "IC_3 = O = IC_9 under the largest signals": ({3: 0, 9: 0}, [R - 1] * 9),
        "vk_x = O through s_1 = -ic_0 / ic_1": ({0: ic0, 1: u}, [-ic0 * inv(u) % R] + [0] * 8),
        "all signals zero": ({}, [0] * 9),
        "all signals zero, IC_0 = O, vk_x = O": ({0: 0}, [0] * 9),
    }


VKX_CASES = _vkx_cases()
VKX_AT_INFINITY = [n for n in VKX_CASES if "vk_x = O" in n]
assert len(VKX_CASES) == 11 and len(VKX_AT_INFINITY) == 3


@pytest.mark.parametrize("name", list(VKX_CASES))
def test_vkx_exceptional_additions(name):
    ic, special = VKX_CASES[name]
    key = Key(9, 510, ic=ic)
    assert (key.ic_log(special) == 0) == (name in VKX_AT_INFINITY)
    if "vk_x = IC_0" in name:
        assert key.ic_log(special) == key.ic[0] != 0
    generic = V._signals(key.rnd, 9, 3)
    pubs = [generic[0], special, generic[1], special, generic[2]]
    logs = key.forge(pubs)
    a, b, c = logs[1]
    logs[3] = (a, b, (c + 1) % R)   # the same row with a changed c
    want = [VALID if key.holds(*l, p) else EQUATION for l, p in zip(logs, pubs)]
    assert want == [VALID, VALID, VALID, EQUATION, VALID]
    assert list(V._verify_both(key, V._proof_rows(logs), pubs)) == want


# -- 6: degenerate keys ---------------------------------------------------------------------------------------------------------------
DEGENERATE = {"gamma2 = O": dict(gamma=0), "delta2 = O": dict(delta=0), "gamma2 = delta2 = O": dict(gamma=0, delta=0), "alpha1 = O": dict(alpha=0),
              "beta2 = O": dict(beta=0), "alpha1 = gamma2 = O": dict(alpha=0, gamma=0), "alpha1 = gamma2 = delta2 = O": dict(alpha=0, gamma=0, delta=0)}


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_keys(name):
    """forged VALID rows and EQUATION rows under keys with points at infinity.  With delta2 = O the forgery solves for b (c is
    free), otherwise for c; with alpha1 = gamma2 = O the row A = O, C = O skips all three pairs and is VALID."""
    key = Key(2, 600, **DEGENERATE[name])
    rnd = key.rnd
    if key.alpha == 0 or key.beta == 0:
        assert key.vk.alphabeta() == BP.gt_bytes(BP.ONE)
    else:
        assert key.vk.alphabeta() == BP.gt_bytes(BP.power(pairing_of_generators(), key.alpha * key.beta % R))
    pubs = V._signals(rnd, 2, 6)
    logs = []
    for i, pub in enumerate(pubs):
        a = rnd.randrange(1, R)
        if key.delta == 0:
            b, c = (key.alpha * key.beta + key.gamma * key.ic_log(pub)) * inv(a) % R, rnd.randrange(1, R)
            if b == 0:   # alpha beta + gamma ic = 0: A B must pair to one, so A = O (B = O is row 4)
                a, b = 0, rnd.randrange(1, R)
        else:
            b = rnd.randrange(1, R)
            c = key.c_for(a, b, pub)
        logs.append((a, b, c))
    if key.delta:
        logs[2] = (0, logs[2][1], key.c_for(0, logs[2][1], pubs[2]))             # A = O
    if key.alpha * key.beta % R == 0 and key.gamma == 0:
        logs[3] = (0, rnd.randrange(1, R), 0)                                     # A = O, C = O: nothing to pair
        logs[4] = (rnd.randrange(1, R), 0, 0)                                     # B = O, C = O
    a, b, c = logs[0]
    logs[1] = (a, (b + 1) % R, c) if key.delta == 0 and a else (a or 1, b, (c + 1) % R)   # a wrong b where c is free, else a wrong c
    logs[5] = (rnd.randrange(1, R), rnd.randrange(1, R), rnd.randrange(1, R))   # unrelated logs
    want = [VALID if key.holds(*l, p) else EQUATION for l, p in zip(logs, pubs)]
    assert want[0] == VALID and want[1] == EQUATION and want[5] == EQUATION and want.count(VALID) == 4
    assert list(V._verify_both(key, V._proof_rows(logs), pubs)) == want
