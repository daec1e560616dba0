"""Groth16 phase-2 contributions on an MI355X (r1cs/contribute.hip, include/graph_witness_groth16_contribute.h).  The oracle of a
chain of contributions is existing code: a key made from a `.ptau` of known (tau, alpha, beta) with delta = 1 and contributed
to with d1, d2 must hold, byte for byte, sections 1 to 9 of groth16_setup(r, (tau, alpha, beta, 1, d1 d2 mod r)).  The two
kernels are tested through their aids on multiples of the generator from bn254_gen_mul_batch_device, so every expected
point is one more fixed-base multiplication; the records against tests/contribution_fixtures.py."""
import functools
import json
import math
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

import cwc_import
from tests import bn254_pairing as BP
from tests import contribution_fixtures as CF
from tests import groth16_fixtures as GF
from tests import ptau_fixtures as PF
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
R, Q = F.R, GF.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "circom-witnesscalc_amd")
_rnd = random.Random(400)
TAU, ALPHA, BETA, D_A, D_B, D_C = (_rnd.randrange(2, R) for _ in range(6))
DELTA_PAIRS = {"r_minus_1_and_2": (R - 1, 2), "random_and_random": (D_A, D_B), "one_and_random": (1, D_C)}
HDR_DELTA1 = 84 + 64 + 64 + 128 + 128
MONT_INV = pow(GF.MONT, -1, Q)

pytestmark = pytest.mark.gpu


# -- files ----------------------------------------------------------------------------------------------------------------------
def sections(zkey):
    """`.zkey` bytes -> ([section ids in file order], {id: body})"""
    assert zkey[:4] == b"zkey" and struct.unpack_from("<I", zkey, 4)[0] == 1
    n_sec = struct.unpack_from("<I", zkey, 8)[0]
    off, ids, out = 12, [], {}
    for _ in range(n_sec):
        sid, size = struct.unpack_from("<IQ", zkey, off)
        off += 12
        ids.append(sid)
        out[sid] = zkey[off:off + size]
        off += size
    assert off == len(zkey)
    return ids, out


def with_sections(zkey, **changed):
    """the key with the bodies of sections s<id> replaced"""
    ids, secs = sections(zkey)
    for k, body in changed.items():
        secs[int(k[1:])] = body
    return b"zkey" + struct.pack("<II", 1, len(ids)) + b"".join(GF.section(i, secs[i]) for i in ids)


def patched(body, at, new):
    return body[:at] + new + body[at + len(new):]


def device_canonical(group, scalars):
    """[k] -> uint8 [n, 64 group]: k G, canonical affine, zero bytes for infinity (existing code)"""
    import torch
    arr = np.frombuffer(b"".join((k % R).to_bytes(32, "little") for k in scalars), dtype=np.uint8).reshape(len(scalars), 32)
    out = PKG.bn254_gen_mul_batch_device(torch.from_numpy(arr.copy()).cuda(), group)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def device_points(group, scalars):
    raw = device_canonical(group, scalars).tobytes()
    return b"".join(GF.lem(int.from_bytes(raw[o:o + 32], "little")) for o in range(0, len(raw), 32))


@functools.lru_cache(maxsize=None)
def ptau(power):
    return PF.assemble(PF.sections(power, TAU, ALPHA, BETA, points=device_points))


# -- the constraint systems of test_gpu_groth16_setup_ptau.py (constructions restated) ------------------------------------------
def _power_system(p):
    n_pub_in = 0 if p <= 2 else 2
    n_pub = n_pub_in + (0 if p <= 2 else 1)
    n_c = (1 << p) - n_pub - 1 - random.Random(p).randrange(0, 1 << (p - 1))
    rnd = random.Random(100 + p)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(n_c)]
    pl = F.planted_system(rnd, 6, shapes, [1, R - 1, 2, F.MONT_R, None])
    return pl.constraints, pl.n_wires, n_pub - n_pub_in, n_pub_in, p


def _column_edges_system():
    n_c, n_wires = 10, 9
    rnd = random.Random(42)
    cons = []
    for k in range(n_c):
        a = [(4, rnd.randrange(1, R))]
        b = [(3, rnd.randrange(1, R))] if k % 3 == 0 else [(0, 1)]
        c = [(2, rnd.randrange(1, R))] if k % 4 == 1 else []
        cons.append((a, b, c))
    cons[2][0].append((5, 9))
    cons[2][2].append((5, -BETA * 9 % R))               # w_5 = -beta u_5, v_5 = 0: the C point of wire 5 is infinity
    cons[6][0].extend([(6, 3), (8, R - 1), (6, 5)])
    cons[7][1].extend([(7, 12345), (8, 2), (7, R - 12345)])
    return cons, n_wires, 0, 0, 4


def _column_skew_system():
    n_c, n_wires = (1 << 10) - 1, 24
    rnd = random.Random(43)
    cons = []
    for k in range(n_c):
        other = 2 + k % (n_wires - 2)
        cons.append(([(1, rnd.randrange(1, R)), (other, 1)], [(1, R - 1), (0, rnd.randrange(R))], [(other, 2), (1, rnd.randrange(1, R))]))
    return cons, n_wires, 0, 0, 10


SYSTEMS = {"p1": functools.partial(_power_system, 1), "p3": functools.partial(_power_system, 3), "p8": functools.partial(_power_system, 8),
           "column_edges": _column_edges_system, "column_skew": _column_skew_system}


@functools.lru_cache(maxsize=None)
def system(name):
    cons, n_wires, n_pub_out, n_pub_in, p = SYSTEMS[name]()
    r1 = PKG.R1cs(F.write_r1cs(n_wires, cons, n_pub_out=n_pub_out, n_pub_in=n_pub_in))
    assert r1.qap_info()["domain_power"] == p
    return p, r1


@functools.lru_cache(maxsize=None)
def key0(name):
    p, r1 = system(name)
    return PKG.groth16_setup_ptau(r1, ptau(p + 1), 1, "compute")


@functools.lru_cache(maxsize=None)
def chain(name, pair):
    """(key0, k1, k2, hash1, hash2)"""
    d1, d2 = DELTA_PAIRS[pair]
    k1, h1 = PKG.groth16_contribute(key0(name), name="first", delta=d1)
    k2, h2 = PKG.groth16_contribute(k1, name="second", delta=d2)
    return key0(name), k1, k2, h1, h2


# -- 1. the scale aid -----------------------------------------------------------------------------------------------------------
SCALE_KS = {"one": 1, "two": 2, "r_minus_1": R - 1, "two_253_plus_1": (1 << 253) + 1, "random": _rnd.randrange(2, R)}


def _scaled(logs, k):
    import torch
    d_in = torch.from_numpy(device_canonical(1, logs)).cuda()
    got = PKG.bn254_g1_scale_batch_device(d_in, k)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("k", list(SCALE_KS))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_scale_aid(n, k):
    """a wave short of one point, a full wave, one more; more than a workgroup; infinity (log 0) in the first, a middle and the
    last slot"""
    rnd = random.Random(1000 + n)
    logs = [rnd.randrange(1, R) for _ in range(n)]
    cases = [logs]
    if n >= 3:
        logs[0] = logs[n // 2] = logs[n - 1] = 0
    else:
        cases.append([0])
    for ks in cases:
        got = _scaled(ks, SCALE_KS[k])
        want = device_canonical(1, [SCALE_KS[k] * x % R for x in ks])
        assert got.shape == want.shape == (len(ks), 64)
        assert np.array_equal(got, want), "rows %s differ" % np.nonzero((got != want).any(axis=1))[0][:8]
        for i, x in enumerate(ks):
            assert got[i].any() == (x != 0)


# -- 2. the linear-combination aid ----------------------------------------------------------------------------------------------
def _lincomb(logs, rhos):
    import torch
    d_in = torch.from_numpy(device_canonical(1, logs)).cuda()
    rho = np.frombuffer(b"".join(x.to_bytes(16, "little") for x in rhos), dtype=np.uint8).reshape(len(rhos), 16)
    got = PKG.bn254_g1_lincomb128_device(d_in, torch.from_numpy(rho.copy()).cuda())
    torch.cuda.synchronize()
    return got.cpu().numpy().tobytes()


@pytest.mark.parametrize("n", (1, 2, 64, 65, 256, 257, 4097))
def test_lincomb_aid(n):
    """one point; a pair; a wave, one more; a workgroup, one more; many workgroups with a last one of one point.  From 64 points
    on the list holds rho = 0, 1 and 2^128 - 1, an infinity point, a pair P, -P and a pair P, P with equal rho, each pair in the
    two slots that the workgroup's tree adds first (32 apart below 256 points, 128 apart from there on)"""
    rnd = random.Random(2000 + n)
    top = (1 << 128) - 1
    logs = [rnd.randrange(1, R) for _ in range(n)]
    rhos = [rnd.randrange(1 << 128) for _ in range(n)]
    if n == 1:
        rhos[0] = top
    elif n == 2:
        logs[1], rhos[1] = R - logs[0], rhos[0]                 # the whole sum cancels
    else:
        gap = 128 if n >= 256 else 32
        rhos[0], rhos[1], rhos[2] = 0, 1, top
        logs[3 + gap], rhos[3 + gap] = logs[3], rhos[3]         # P + P: the doubling branch
        logs[5 + gap], rhos[5 + gap] = R - logs[5], rhos[5]     # P + (-P)
        logs[7] = 0                                             # infinity with a nonzero rho
        rhos[n - 1] = top
    want = device_canonical(1, [sum(r * k for r, k in zip(rhos, logs)) % R]).tobytes()
    assert _lincomb(logs, rhos) == want
    if n == 2:
        assert want == bytes(64)


def test_lincomb_aid_all_zero():
    rnd = random.Random(2100)
    assert _lincomb([rnd.randrange(1, R) for _ in range(65)], [0] * 65) == bytes(64)


# -- 3. byte parity with the trapdoor setup -------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", list(DELTA_PAIRS))
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_chain_is_the_trapdoor_key(name, pair):
    _, r1 = system(name)
    d1, d2 = DELTA_PAIRS[pair]
    k0, k1, k2, _, _ = chain(name, pair)
    ids, got = sections(k2)
    assert ids == list(range(1, 11))
    _, want = sections(PKG.groth16_setup(r1, (TAU, ALPHA, BETA, 1, d1 * d2 % R)))
    for sid in range(1, 10):
        assert got[sid] == want[sid], "section %d differs" % sid
    _, s0 = sections(k0)
    assert got[4] == s0[4]
    assert sections(k1)[0] == list(range(1, 11))
    if name == "column_edges":
        assert not any(got[8][64 * 4:64 * 5]) and not any(got[8][:64]) and any(got[8][64:128])  # wires 5 and 1: infinity stays
    info = PKG.zkey_contributions(k2)
    assert [c["name"] for c in info["contributions"]] == ["first", "second"]


def test_chain_in_small_pieces(monkeypatch):
    """CWC_CONTRIBUTE_CHUNK = 100: sections 8 and 9 of p8 (more than 256 points) in several pieces, the last one short"""
    k0, k1, _, _, _ = chain("p8", "random_and_random")
    monkeypatch.setenv("CWC_CONTRIBUTE_CHUNK", "100")
    again, _ = PKG.groth16_contribute(k0, name="first", delta=D_A)
    _, a = sections(again)
    _, b = sections(k1)
    assert len(a[8]) // 64 + len(a[9]) // 64 > 256
    assert all(a[s] == b[s] for s in range(1, 10))
    PKG.groth16_verify_contribution_step(k0, again, seed=bytes(32))
    bad = with_sections(again, s9=patched(a[9], len(a[9]) - 64, GF.g1_bytes(GF.G1_GEN)))
    with pytest.raises(PKG.WitnessCalcError, match=r"section 9 \(H\)"):
        PKG.groth16_verify_contribution_step(k0, bad, seed=bytes(32))


# -- 4. the record --------------------------------------------------------------------------------------------------------------
def _pairings(pairs):
    """[(G1 affine, G2 affine)] -> [384 bytes], on the device: a pairing of tests/bn254_pairing.py takes seconds in pure Python,
    and bn254_pairing_batch_device is existing code with tests of its own against it"""
    import torch
    g1 = np.frombuffer(b"".join(CF.canonical_g1(p) for p, _ in pairs), dtype=np.uint8).reshape(len(pairs), 64)
    g2 = np.frombuffer(b"".join(CF.canonical_g2(q) for _, q in pairs), dtype=np.uint8).reshape(len(pairs), 128)
    gt = PKG.bn254_pairing_batch_device(torch.from_numpy(g1.copy()).cuda(), torch.from_numpy(g2.copy()).cuda())
    torch.cuda.synchronize()
    return [bytes(row) for row in gt.cpu().numpy()]


def test_record_is_the_python_record():
    d1, _ = DELTA_PAIRS["random_and_random"]
    k0, k1, _, h1, _ = chain("p1", "random_and_random")
    _, s0 = sections(k0)
    _, s1 = sections(k1)
    assert s0[10] == CF.NO_RECORDS
    cs_hash, recs = CF.read_section10(s1[10])
    assert cs_hash == CF.H(b"".join(s0[i] for i in range(1, 10))) and len(recs) == 1
    got = recs[0]
    assert got.g1_s is not None and GF.G1.on_curve(got.g1_s)
    t = CF.transcript(cs_hash, [], got.g1_s, GF.G1.to_affine(GF.G1.mul(got.g1_s, d1)))
    sp = CF.hash_to_g2(t)
    want = CF.Record(GF.G1.to_affine(GF.G1.gen_mul_jac(d1)), got.g1_s, GF.G1.to_affine(GF.G1.mul(got.g1_s, d1)),
                     GF.G2.to_affine(GF.G2.mul(sp, d1)), t, 0, CF.name_params("first"))
    assert got.stored() == want.stored()
    assert h1 == want.hash() == PKG.zkey_contributions(k1)["contributions"][0]["hash"]
    assert s1[2][HDR_DELTA1:HDR_DELTA1 + 64] == GF.g1_bytes(want.delta_after)
    gt = _pairings([(got.g1_s, got.g2_spx), (got.g1_sx, sp), (GF.G1_GEN, got.g2_spx), (got.delta_after, sp)])
    assert gt[0] == gt[1] and gt[2] == gt[3] and gt[0] != gt[2]


# -- 5. groth16_verify_contributions --------------------------------------------------------------------------------------------
def test_verify_contributions_accepts_the_chain():
    k0, k1, k2, h1, h2 = chain("p3", "random_and_random")
    assert PKG.groth16_verify_contributions(k0) == []
    assert PKG.groth16_verify_contributions(k1) == [h1]
    assert PKG.groth16_verify_contributions(k2) == [h1, h2]
    assert h1 != h2


def test_verify_contributions_refusals():
    _, r1 = system("p3")
    _, _, k2, _, _ = chain("p3", "random_and_random")
    with pytest.raises(PKG.WitnessCalcError, match="^zkey: delta is not the generator and no contribution accounts for it$"):
        PKG.groth16_verify_contributions(PKG.groth16_setup(r1, (TAU, ALPHA, BETA, 1, 5)))
    _, s = sections(k2)
    cs_hash, recs = CF.read_section10(s[10])
    # records swapped: the first one's transcript no longer fits
    swapped = with_sections(k2, s10=CF.write_section10(cs_hash, recs[::-1]))
    with pytest.raises(PKG.WitnessCalcError, match="^zkey: contribution 1: the transcript"):
        PKG.groth16_verify_contributions(swapped)
    # one transcript byte flipped
    at = 68 + len(recs[0].stored()) + 320 + 17
    flipped = with_sections(k2, s10=patched(s[10], at, bytes([s[10][at] ^ 1])))
    with pytest.raises(PKG.WitnessCalcError, match="^zkey: contribution 2: the transcript"):
        PKG.groth16_verify_contributions(flipped)
    # g2_spx of the last record on the twist, outside the subgroup
    out = BP.twist_point_outside_subgroup(random.Random(9))
    moved = CF.Record(recs[1].delta_after, recs[1].g1_s, recs[1].g1_sx, out, recs[1].transcript, 0, recs[1].params)
    with pytest.raises(PKG.WitnessCalcError, match="^zkey: contribution 2: g2_spx is not in the order-r subgroup of G2$"):
        PKG.groth16_verify_contributions(with_sections(k2, s10=CF.write_section10(cs_hash, [recs[0], moved])))
    # g2_spx another multiple of the challenge: the proof of knowledge fails
    other = CF.Record(recs[0].delta_after, recs[0].g1_s, recs[0].g1_sx, GF.G2.to_affine(GF.G2.mul(recs[0].g2_spx, 2)), recs[0].transcript, 0,
                      recs[0].params)
    with pytest.raises(PKG.WitnessCalcError, match="^zkey: contribution 1: g1_sx is not g1_s times the secret"):
        PKG.groth16_verify_contributions(with_sections(k2, s10=CF.write_section10(cs_hash, [other, recs[1]])))
    # delta2 another multiple of the G2 generator
    d2 = GF.g2_bytes(GF.G2.to_affine(GF.G2.gen_mul_jac(12345)))
    with pytest.raises(PKG.WitnessCalcError, match="^zkey: delta2 is not the G2 generator times delta1's scalar$"):
        PKG.groth16_verify_contributions(with_sections(k2, s2=patched(s[2], HDR_DELTA1 + 64, d2)))
    # delta1 not the last deltaAfter
    with pytest.raises(PKG.WitnessCalcError, match="^zkey: delta1 is not the deltaAfter of the last contribution$"):
        PKG.groth16_verify_contributions(with_sections(k2, s2=patched(s[2], HDR_DELTA1, GF.g1_bytes(recs[0].delta_after))))


# -- 6. groth16_verify_contribution_step ----------------------------------------------------------------------------------------
def _stored_to_canonical(body):
    return np.frombuffer(b"".join((int.from_bytes(body[o:o + 32], "little") * MONT_INV % Q).to_bytes(32, "little") for o in range(0, len(body), 32)),
                         dtype=np.uint8).reshape(-1, 64)


def _scale_stored(body, k):
    """every stored G1 point of `body` times k, through the scale aid"""
    import torch
    got = PKG.bn254_g1_scale_batch_device(torch.from_numpy(_stored_to_canonical(body).copy()).cuda(), k)
    torch.cuda.synchronize()
    raw = got.cpu().numpy().tobytes()
    return b"".join(GF.lem(int.from_bytes(raw[o:o + 32], "little")) for o in range(0, len(raw), 32))


def test_verify_step_accepts_the_chain():
    k0, k1, k2, _, _ = chain("p8", "random_and_random")
    for seed in (bytes(32), bytes(range(32)), None):
        PKG.groth16_verify_contribution_step(k0, k1, seed=seed)
        PKG.groth16_verify_contribution_step(k1, k2, seed=seed)
    e0, e1, _, _, _ = chain("column_edges", "r_minus_1_and_2")  # a C point at infinity
    PKG.groth16_verify_contribution_step(e0, e1)


def test_verify_step_refusals():
    k0, k1, k2, _, _ = chain("p8", "random_and_random")
    _, s = sections(k2)
    gen = GF.g1_bytes(GF.G1_GEN)
    seed = bytes(range(1, 33))

    def refused(nxt, pattern, prev=k1):
        with pytest.raises(PKG.WitnessCalcError, match=pattern):
            PKG.groth16_verify_contribution_step(prev, nxt, seed=seed)

    n_c, n_h = len(s[8]) // 64, len(s[9]) // 64
    assert n_c > 2 and n_h == 256
    refused(with_sections(k2, s8=patched(s[8], 64 * (n_c // 2), gen)), r"^zkey step: section 8 \(C\) is not")
    refused(with_sections(k2, s9=patched(s[9], 64 * (n_h - 1), _scale_stored(s[9][-64:], 2))), r"^zkey step: section 9 \(H\) is not")
    refused(with_sections(k2, s8=_scale_stored(s[8], 3), s9=_scale_stored(s[9], 3)), r"^zkey step: section 8 \(C\) is not")
    refused(with_sections(k2, s9=_scale_stored(s[9], 3)), r"^zkey step: section 9 \(H\) is not")
    refused(with_sections(k2, s5=patched(s[5], 64 * 3, gen)), r"^zkey step: section 5 \(A\) differs")
    value_at = 4 + 44 * 2 + 12
    refused(with_sections(k2, s4=patched(s[4], value_at, bytes([s[4][value_at] ^ 1]))), r"^zkey step: section 4 \(coefficients\) differs")
    refused(with_sections(k2, s2=patched(s[2], 84, gen)), r"^zkey step: section 2 \(header\) differs")
    refused(k2, r"^zkey step: section 10 of the next key has 2 contributions, the previous key 0", prev=k0)
    refused(k1, r"^zkey step: section 10 of the next key has 1 contributions, the previous key 1")
    cs_hash, recs = CF.read_section10(s[10])
    refused(with_sections(k2, s10=CF.write_section10(bytes(64), recs)), r"^zkey step: section 10: the csHash is not the previous key's$")
    _, s1 = sections(k1)
    other_hash = with_sections(k1, s10=patched(s1[10], 5, bytes([s1[10][5] ^ 1])))
    refused(other_hash, r"^zkey step: section 10: the csHash is not the hash of the previous key's sections 1 to 9$", prev=k0)
    first = CF.Record(recs[0].delta_after, recs[0].g1_s, recs[0].g1_sx, recs[0].g2_spx, recs[0].transcript, 0, CF.name_params("other"))
    refused(with_sections(k2, s10=CF.write_section10(cs_hash, [first, recs[1]])), r"^zkey step: section 10: contribution 1 is not the previous key's$")
    # the new record's own rules, with deltaPrev the previous key's delta1: a next key whose delta1 moved
    _, sa = sections(chain("p8", "one_and_random")[2])
    refused(with_sections(k2, s2=patched(s[2], HDR_DELTA1, sa[2][HDR_DELTA1:HDR_DELTA1 + 64])), r"^zkey: delta1 is not the deltaAfter of the last contribution$")


# -- 7. a drawn secret ----------------------------------------------------------------------------------------------------------
def test_drawn_secret_and_proofs():
    rnd = random.Random(46)
    shapes = [{"a": rnd.randrange(1, 4), "b": rnd.randrange(1, 4), "c": rnd.randrange(0, 3)} for _ in range(50)]
    pl = F.planted_system(rnd, 6, shapes, [1, R - 1, 2, F.MONT_R, None])
    r1 = PKG.R1cs(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=2))
    k0 = PKG.groth16_setup_ptau(r1, ptau(7), 1)
    (ka, ha), (kb, hb) = PKG.groth16_contribute(k0), PKG.groth16_contribute(k0, name="b")
    assert ka != kb and ha != hb
    _, sa = sections(ka)
    _, sb = sections(kb)
    assert sa[2][HDR_DELTA1:] != sb[2][HDR_DELTA1:] and sa[8] != sb[8] and sa[9] != sb[9] and sa[5] == sb[5]
    assert PKG.groth16_verify_contributions(ka) == [ha] and PKG.groth16_verify_contributions(kb) == [hb]
    PKG.groth16_verify_contribution_step(k0, ka)
    g = PKG.Groth16(ka)
    rows = [pl.complete(random.Random(47 + i)) for i in range(4)]
    proofs = g.prove_batch(F.rows_array(rows))
    publics = [w[1:4] for w in rows]
    assert list(g.verifying_key().verify_batch(proofs, publics)) == [PKG.VERIFY_VALID] * 4
    assert list(PKG.Groth16VerifyingKey.from_zkey(k0).verify_batch(proofs, publics)) == [PKG.VERIFY_EQUATION] * 4


# -- 8. the CLI chain -----------------------------------------------------------------------------------------------------------
def _wtns(w):
    img = b"wtns" + struct.pack("<II", 2, 2)
    img += struct.pack("<IQI", 1, 40, 32) + R.to_bytes(32, "little") + struct.pack("<I", len(w))
    return img + struct.pack("<IQ", 2, 32 * len(w)) + b"".join(x.to_bytes(32, "little") for x in w)


def test_cli_chain(tmp_path):
    """groth16-setup --ptau --delta 1, two contributions, --verify, --verify-step, groth16-prove, groth16-verify; every step under
    its own time limit, and the first failure ends the chain"""
    rnd = random.Random(46)
    shapes = [{"a": rnd.randrange(1, 4), "b": rnd.randrange(1, 4), "c": rnd.randrange(0, 3)} for _ in range(50)]
    pl = F.planted_system(rnd, 6, shapes, [1, R - 1, 2, F.MONT_R, None])
    (tmp_path / "c.r1cs").write_bytes(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=2))
    (tmp_path / "pot.ptau").write_bytes(ptau(7))
    (tmp_path / "one.txt").write_text("1\n")
    (tmp_path / "d.txt").write_text("%d\n" % D_A)
    (tmp_path / "w.wtns").write_bytes(_wtns(pl.complete(random.Random(50))))
    path = lambda name: str(tmp_path / name)  # noqa: E731

    def run(tool, *args):
        p = subprocess.run([os.path.join(BIN, tool)] + list(args), capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (tool, args, p.returncode, p.stdout, p.stderr)
        return p.stdout

    run("groth16-setup", "--ptau", path("pot.ptau"), "--delta", path("one.txt"), path("c.r1cs"), path("k0.zkey"))
    h1 = run("groth16-contribute", "--name", "first", "--delta", path("d.txt"), path("k0.zkey"), path("k1.zkey")).strip()
    h2 = run("groth16-contribute", "--name", "second", path("k1.zkey"), path("k2.zkey")).strip()
    k0, k1, k2 = ((tmp_path / n).read_bytes() for n in ("k0.zkey", "k1.zkey", "k2.zkey"))
    want1, want_hash = PKG.groth16_contribute(k0, name="first", delta=D_A)
    assert sections(k1)[1][8] == sections(want1)[1][8] and len(h1) == 128 and len(h2) == 128
    assert [c["name"] for c in PKG.zkey_contributions(k2)["contributions"]] == ["first", "second"]
    assert [c["hash"].hex() for c in PKG.zkey_contributions(k2)["contributions"]] == [h1, h2]
    out = run("groth16-contribute", "--verify", path("k2.zkey"))
    assert "OK!" in out and h1 in out and h2 in out
    assert "OK!" in run("groth16-contribute", "--verify-step", path("k1.zkey"), path("k2.zkey"))
    p = subprocess.run([os.path.join(BIN, "groth16-contribute"), "--verify-step", path("k0.zkey"), path("k2.zkey")], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 1 and "INVALID: zkey step: section 10" in p.stderr
    (tmp_path / "vk.json").write_text(json.dumps(PKG.Groth16VerifyingKey.from_zkey(k2).to_json()))
    run("groth16-prove", path("c.r1cs"), path("k2.zkey"), path("w.wtns"), path("proof.json"), path("public.json"))
    assert "OK!" in run("groth16-verify", path("vk.json"), path("public.json"), path("proof.json"))


# -- 9. the phase timer ---------------------------------------------------------------------------------------------------------
_TIMER_SCRIPT = """
import sys
sys.path.insert(0, %r)
import cwc_import
PKG = cwc_import.load()
try:
    PKG.groth16_contribute_phase_ms()
    print("no refusal")
except PKG.WitnessCalcError as e:
    print("refused:", e)
PKG.groth16_contribute(open(sys.argv[1], "rb").read(), delta=7)
ms = PKG.groth16_contribute_phase_ms()
print("phases:", " ".join("%%s=%%r" %% kv for kv in ms.items()))
"""


def test_phase_timer(tmp_path):
    """a fresh process: nothing to report before the first contribution, three times after it"""
    (tmp_path / "k0.zkey").write_bytes(key0("p3"))
    (tmp_path / "timer.py").write_text(_TIMER_SCRIPT % ROOT)
    p = subprocess.run([sys.executable, str(tmp_path / "timer.py"), str(tmp_path / "k0.zkey")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p
    assert "refused: no contribution phase times" in p.stdout
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("phases:")][0]
    ms = dict((kv.split("=")[0], float(kv.split("=")[1])) for kv in line.split()[1:])
    assert list(ms) == list(PKG.GROTH16_CONTRIBUTE_PHASES) and len(ms) == 3
    assert all(math.isfinite(x) and x >= 0 for x in ms.values()) and ms["scale"] > 0
