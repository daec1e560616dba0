"""The random beacon of both ceremony phases on an MI355X (include/graph_witness_groth16_beacon.h): a beacon is a contribution at
derived scalars, so the oracle of its bytes is the oracle of a contribution: the Python writers of tests/ptau_fixtures.py and the
trapdoor setup for the points, tests/beacon_fixtures.py (hashlib) for the scalars and the records.  Whole output files are
compared byte for byte, on a file of power 3 and on the system of the domain 2^2 (the constructions of
tests/test_gpu_groth16_contribute.py, restated); the verifications accept the honest files and name the beacon rule for each
tampering that only it can catch."""
import ctypes
import functools
import json
import math
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import cwc_import
from tests import beacon_fixtures as BF
from tests import ceremony_fixtures as CE
from tests import contribution_fixtures as CF
from tests import groth16_fixtures as GF
from tests import ptau_fixtures as PF
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
R = GF.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "circom-witnesscalc_amd")
SEED = bytes(range(7, 39))
POWER, EXP = 3, 10
HASH = bytes.fromhex("00000000000000000001a1b2c3d4e5f60718293a4b5c6d7e8f90a1b2c3d4e5f6")  # the shape of a block hash
_rnd = random.Random(1100)
TAU, ALPHA, BETA, D_A, D_B, D_C = (_rnd.randrange(2, R) for _ in range(6))
FIRST, SECOND, ARBITRARY = (tuple(_rnd.randrange(2, R) for _ in range(3)) for _ in range(3))
HDR_DELTA1 = 84 + 64 + 64 + 128 + 128
KEY_RULE = "the key is not the one its beaconHash and numIterationsExp give"
NOT_A_BEACON = "the last contribution is not a beacon"

pytestmark = pytest.mark.gpu


# -- files ----------------------------------------------------------------------------------------------------------------------
def split(image):
    """[(id, body)] of a binfile in file order"""
    (n,), off, out = struct.unpack_from("<I", image, 8), 12, []
    for _ in range(n):
        sid, size = struct.unpack_from("<IQ", image, off)
        out.append((sid, image[off + 12:off + 12 + size]))
        off += 12 + size
    assert off == len(image)
    return out


def join(magic, sections):
    return magic + struct.pack("<II", 1, len(sections)) + b"".join(GF.section(i, b) for i, b in sections)


def with_section(image, sid, body):
    return join(image[:4], [(i, body if i == sid else b) for i, b in split(image)])


def products(*triples):
    return tuple(math.prod(t[j] for t in triples) % R for j in range(3))


def verdict(call, *args):
    """(rc, message) of a verification through the C ABI"""
    st = PKG.GwStatus()
    rc = call(*args, ctypes.byref(st))
    msg = ctypes.string_at(st.error_msg).decode() if st.error_msg else ""
    return rc, msg


def refused(call, *args, **kw):
    with pytest.raises(PKG.WitnessCalcError) as e:
        call(*args, **kw)
    return str(e.value)


# -- phase 1 --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain1():
    """ptau_new, two contributions and the beacon: [(file, digest)]"""
    f0 = PKG.ptau_new(POWER)
    f1, d1 = PKG.ptau_contribute(f0, name="first", secrets=FIRST)
    f2, d2 = PKG.ptau_contribute(f1, name="second", secrets=SECOND)
    fb, db = PKG.ptau_beacon(f2, HASH, EXP, name="beacon")
    return (f0, None), (f1, d1), (f2, d2), (fb, db)


def expected_ptau(before, logs, name):
    """the whole file that ptau_beacon(before, HASH, EXP, name) has to give, `before` a file of the logs `logs` with sections 1 to 7
    in order: sections 1 to 6 of the Python writer for the products, section 7 = the earlier records and the fixture's beacon"""
    secs = dict(split(before))
    x = BF.scalars(1, HASH, EXP)
    want = PF.sections(POWER, *products(logs, x[:3]))
    (n,) = struct.unpack_from("<I", secs[7], 0)
    earlier = CE.read_section7(secs[7])
    challenge = earlier[-1].next_challenge if earlier else CE.first_challenge(secs[1])
    rec = BF.ptau_beacon_record(challenge, logs, HASH, EXP, name)
    assert rec.type == 1 and rec.params == CF.beacon_params(name, EXP, HASH) and rec.partial_hash == bytes(216)
    body7 = struct.pack("<I", n + 1) + secs[7][4:] + rec.stored()
    return join(b"ptau", [(1, secs[1])] + [(sid, want[sid]) for sid in range(2, 7)] + [(7, body7)]), rec


def test_phase1_beacon_bytes():
    (f0, _), _, (f2, _), (fb, db) = chain1()
    # on a new file, without a name: the item 01 is omitted
    out, digest = PKG.ptau_beacon(f0, HASH, EXP)
    want, rec = expected_ptau(f0, (1, 1, 1), "")
    assert out == want and digest == rec.next_challenge
    assert rec.params == bytes([2, EXP, 3, len(HASH)]) + HASH
    # on top of two contributions
    want, rec = expected_ptau(f2, products(FIRST, SECOND), "beacon")
    assert fb == want and db == rec.next_challenge
    got = PKG.ptau_contributions(fb)
    assert [(r["type"], r["iterations_exp"], r["beacon_hash"]) for r in got] == [(0, None, None), (0, None, None), (1, EXP, HASH)]
    assert got[2]["name"] == "beacon" and got[2]["next_challenge"] == db
    # a second run gives the same bytes; a prepared input loses sections 12 to 15
    assert PKG.ptau_beacon(f2, HASH, EXP, name="beacon") == (fb, db)
    prepared = PKG.ptau_prepare_phase2(f2)
    assert PKG.ptau_info(prepared)["prepared"] and {12, 13, 14, 15} <= {sid for sid, _ in split(prepared)}
    out, digest = PKG.ptau_beacon(prepared, HASH, EXP, name="beacon")
    assert [sid for sid, _ in split(out)] == [1, 2, 3, 4, 5, 6, 7] and (out, digest) == (fb, db)
    # the timer reports the call like a contribution
    ms = PKG.ptau_contribute_phase_ms()
    assert list(ms) == list(PKG.PTAU_CONTRIBUTE_PHASES) and all(math.isfinite(x) and x > 0 for x in ms.values())


def rewritten(image, k, change):
    """`image` with record k (0-based) of section 7 changed by change(record); the parameters and the type are in no hash"""
    secs = dict(split(image))
    recs = CE.read_section7(secs[7])
    change(recs[k])
    return with_section(image, 7, CE.write_section7(recs))


def flip_hash_bit(rec):
    rec.params = rec.params[:-1] + bytes([rec.params[-1] ^ 1])


def eleven(rec):
    """numIterationsExp 10 -> 11: item 02 follows the name's item 01, if there is one"""
    at = 2 + rec.params[1] if rec.params[0] == 1 else 0
    assert rec.params[at] == 2 and rec.params[at + 1] == EXP
    rec.params = rec.params[:at + 1] + bytes([EXP + 1]) + rec.params[at + 2:]


def unmark(rec):
    rec.type = 0


def ptau_verify_rc(image):
    n = ctypes.c_size_t(0)
    return verdict(PKG.r1cs_lib().gwb_ptau_verify, image, len(image), 0, SEED, None, ctypes.byref(n))


def ptau_step_rc(prev, nxt):
    return verdict(PKG.r1cs_lib().gwb_ptau_verify_step, prev, len(prev), nxt, len(nxt), SEED)


def test_phase1_beacon_verdicts():
    (f0, _), (_, d1), (f2, d2), (fb, db) = chain1()
    assert PKG.ptau_verify(fb, seed=SEED) == [d1, d2, db] == PKG.ptau_verify(fb, seed=SEED, require_beacon=True)
    PKG.ptau_verify_step(f2, fb, seed=SEED)
    assert NOT_A_BEACON in refused(PKG.ptau_verify, f2, seed=SEED, require_beacon=True)
    assert "ptau: " + NOT_A_BEACON == refused(PKG.ptau_verify, f0, seed=SEED, require_beacon=True)
    want = "ptau: contribution 3: the key of secret tau is not the one its beaconHash and numIterationsExp give"
    for change in (flip_hash_bit, eleven):
        bad = rewritten(fb, 2, change)
        assert ptau_verify_rc(bad) == (1, want), change.__name__
        assert ptau_step_rc(f2, bad) == (1, want), change.__name__
    # a consistent file and record from arbitrary secrets, marked as a beacon: its proofs of knowledge hold
    secs = PF.sections(POWER, *ARBITRARY)
    rec = BF.as_beacon(CE.contribution(CE.first_challenge(secs[1]), (1, 1, 1), ARBITRARY, (3, 5, 7)), "", EXP, HASH)
    secs[7] = CE.write_section7([rec])
    forged = PF.assemble(secs)
    want = "ptau: contribution 1: the key of secret tau is not the one its beaconHash and numIterationsExp give"
    assert ptau_verify_rc(forged) == (1, want) and ptau_step_rc(f0, forged) == (1, want)
    rec.type = 0
    secs[7] = CE.write_section7([rec])
    assert PKG.ptau_verify(PF.assemble(secs), seed=SEED) == [rec.next_challenge]  # the same record as a contribution is accepted
    # the honest beacon marked as a contribution is one; a contribution after a beacon is accepted: neither ends on a beacon
    plain = rewritten(fb, 2, unmark)
    assert PKG.ptau_verify(plain, seed=SEED) == [d1, d2, db]
    assert "ptau: " + NOT_A_BEACON == refused(PKG.ptau_verify, plain, seed=SEED, require_beacon=True)
    after, da = PKG.ptau_contribute(fb, secrets=FIRST)
    assert PKG.ptau_verify(after, seed=SEED) == [d1, d2, db, da]
    PKG.ptau_verify_step(fb, after, seed=SEED)
    assert "ptau: " + NOT_A_BEACON == refused(PKG.ptau_verify, after, seed=SEED, require_beacon=True)


# -- phase 2: the system of tests/test_gpu_groth16_contribute.py for the domain 2^2 and its file, of power 3 -----------------------------
def device_points(group, scalars):
    """[k] -> the stored form of k G, through bn254_gen_mul_batch_device (existing code)"""
    import torch
    arr = np.frombuffer(b"".join((k % R).to_bytes(32, "little") for k in scalars), dtype=np.uint8).reshape(len(scalars), 32)
    out = PKG.bn254_gen_mul_batch_device(torch.from_numpy(arr.copy()).cuda(), group)
    torch.cuda.synchronize()
    raw = out.cpu().numpy().tobytes()
    return b"".join(GF.lem(int.from_bytes(raw[o:o + 32], "little")) for o in range(0, len(raw), 32))


@functools.lru_cache(maxsize=None)
def ptau():
    return PF.assemble(PF.sections(POWER, TAU, ALPHA, BETA, points=device_points))


@functools.lru_cache(maxsize=None)
def system():
    """_power_system(2) of that file: (the planted system, R1cs)"""
    p = 2
    n_c = (1 << p) - 1 - random.Random(p).randrange(0, 1 << (p - 1))
    rnd = random.Random(100 + p)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(n_c)]
    pl = F.planted_system(rnd, 6, shapes, [1, R - 1, 2, F.MONT_R, None])
    r1 = PKG.R1cs(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=0, n_pub_in=0))
    assert r1.qap_info()["domain_power"] == p
    return pl, r1


@functools.lru_cache(maxsize=None)
def chain2():
    """the key with delta = 1, two contributions and the beacon: [(key, hash)]"""
    k0 = PKG.groth16_setup_ptau(system()[1], ptau(), 1, "compute")
    k1, h1 = PKG.groth16_contribute(k0, name="first", delta=D_A)
    k2, h2 = PKG.groth16_contribute(k1, name="second", delta=D_B)
    kb, hb = PKG.groth16_beacon(k2, HASH, EXP, name="beacon")
    return (k0, None), (k1, h1), (k2, h2), (kb, hb)


def test_phase2_beacon_bytes():
    _, r1 = system()
    (k0, _), _, (k2, _), (kb, hb) = chain2()
    delta_b = BF.scalars(2, HASH, EXP)[0]
    got, s2 = split(kb), dict(split(k2))
    assert [sid for sid, _ in got] == list(range(1, 11))
    want = dict(split(PKG.groth16_setup(r1, (TAU, ALPHA, BETA, 1, D_A * D_B * delta_b % R))))
    for sid, body in got[:9]:
        assert body == want[sid], "section %d differs" % sid
    cs_hash, before = CF.read_section10(s2[10])
    rec = BF.zkey_beacon_record(cs_hash, before, GF.G1.to_affine(GF.G1.gen_mul_jac(D_A * D_B % R)), HASH, EXP, "beacon")
    assert rec.type == 1 and rec.params == CF.beacon_params("beacon", EXP, HASH)
    assert dict(got)[10] == s2[10][:64] + struct.pack("<I", 3) + s2[10][68:] + rec.stored() and hb == rec.hash()
    info = PKG.zkey_contributions(kb)["contributions"]
    assert [(c["type"], c["iterations_exp"], c["beacon_hash"]) for c in info] == [(0, None, None), (0, None, None), (1, EXP, HASH)]
    assert PKG.groth16_beacon(k2, HASH, EXP, name="beacon") == (kb, hb)
    ms = PKG.groth16_contribute_phase_ms()
    assert list(ms) == list(PKG.GROTH16_CONTRIBUTE_PHASES) and ms["scale"] > 0
    # on a blank key the first record sets the csHash
    s0 = dict(split(k0))
    assert s0[10] == CF.NO_RECORDS
    first, hf = PKG.groth16_beacon(k0, HASH, EXP)
    cs_hash = CF.H(b"".join(s0[i] for i in range(1, 10)))
    rec = BF.zkey_beacon_record(cs_hash, [], GF.G1_GEN, HASH, EXP)
    assert dict(split(first))[10] == CF.write_section10(cs_hash, [rec]) and hf == rec.hash()
    want = dict(split(PKG.groth16_setup(r1, (TAU, ALPHA, BETA, 1, delta_b))))
    assert all(dict(split(first))[sid] == want[sid] for sid in range(1, 10))


def rewritten_key(key, k, change):
    secs = dict(split(key))
    cs_hash, recs = CF.read_section10(secs[10])
    change(recs[k])
    return with_section(key, 10, CF.write_section10(cs_hash, recs))


def zkey_rcs(prev, key):
    """(rc, message) of the three verifications of `key`, the step from `prev`"""
    L, r1 = PKG.r1cs_lib(), system()[1]
    n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
    return (verdict(L.gwb_zkey_verify_contributions, key, len(key), None, ctypes.byref(n)),
            verdict(L.gwb_zkey_verify_step, prev, len(prev), key, len(key), SEED),
            verdict(L.gwb_zkey_verify_key, key, len(key), r1._h, ptau(), len(ptau()), PKG.PTAU_LAGRANGE_MODES["compute"], 0, SEED, None, ctypes.byref(m)))


def test_phase2_beacon_verdicts():
    _, r1 = system()
    _, (_, h1), (k2, h2), (kb, hb) = chain2()
    assert PKG.groth16_verify_contributions(kb) == [h1, h2, hb] == PKG.groth16_verify_contributions(kb, require_beacon=True)
    PKG.groth16_verify_contribution_step(k2, kb, seed=SEED)
    assert PKG.groth16_verify_key(kb, r1, ptau(), seed=SEED, require_beacon=True) == [h1, h2, hb]
    assert "zkey: " + NOT_A_BEACON == refused(PKG.groth16_verify_contributions, k2, require_beacon=True)
    assert "zkey: " + NOT_A_BEACON == refused(PKG.groth16_verify_key, k2, r1, ptau(), seed=SEED, require_beacon=True)
    # a real third contribution marked as a beacon: the key is consistent and its proof of knowledge holds
    k3, h3 = PKG.groth16_contribute(k2, name="third", delta=D_C)
    forged = rewritten_key(k3, 2, lambda rec: BF.as_beacon(rec, "third", EXP, HASH))
    for bad in (rewritten_key(kb, 2, flip_hash_bit), rewritten_key(kb, 2, eleven), forged):
        assert zkey_rcs(k2, bad) == ((1, "zkey: contribution 3: " + KEY_RULE), (1, "zkey: contribution 3: " + KEY_RULE),
                                     (1, "zkey verify: contribution 3: " + KEY_RULE))
    # the honest beacon marked as a contribution is one; a contribution after a beacon is accepted: neither ends on a beacon
    plain = rewritten_key(kb, 2, unmark)
    assert zkey_rcs(k2, plain) == ((0, ""), (0, ""), (0, ""))
    assert "zkey: " + NOT_A_BEACON == refused(PKG.groth16_verify_contributions, plain, require_beacon=True)
    assert "zkey: " + NOT_A_BEACON == refused(PKG.groth16_verify_key, plain, r1, ptau(), seed=SEED, require_beacon=True)
    after, ha = PKG.groth16_contribute(kb, delta=D_C)
    assert PKG.groth16_verify_contributions(after) == [h1, h2, hb, ha]
    assert "zkey: " + NOT_A_BEACON == refused(PKG.groth16_verify_contributions, after, require_beacon=True)


# -- the shell chain ------------------------------------------------------------------------------------------------------------
def _wtns(w):
    img = b"wtns" + struct.pack("<II", 2, 2)
    img += struct.pack("<IQI", 1, 40, 32) + R.to_bytes(32, "little") + struct.pack("<I", len(w))
    return img + struct.pack("<IQ", 2, 32 * len(w)) + b"".join(x.to_bytes(32, "little") for x in w)


def _run(tool, *args):
    return subprocess.run([os.path.join(BIN, tool)] + list(args), capture_output=True, text=True, timeout=120)


def _ok(tool, *args):
    p = _run(tool, *args)
    assert p.returncode == 0, (tool, args, p.returncode, p.stdout, p.stderr)
    return p.stdout


def test_cli_chain_from_a_new_file_to_a_verified_proof(tmp_path):
    """every step a child under its own time limit; the first failure ends the chain"""
    pl, _ = system()
    path = lambda name: str(tmp_path / name)  # noqa: E731
    (tmp_path / "c.r1cs").write_bytes(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=0, n_pub_in=0))
    (tmp_path / "s.txt").write_text(" ".join(str(x) for x in FIRST) + "\n")
    (tmp_path / "one.txt").write_text("1\n")
    (tmp_path / "d.txt").write_text("%d\n" % D_A)
    (tmp_path / "w.wtns").write_bytes(_wtns(pl.complete(random.Random(51))))
    _ok("powersoftau", "new", str(POWER), path("f0.ptau"))
    _ok("powersoftau", "contribute", "--name", "first", "--secrets", path("s.txt"), path("f0.ptau"), path("f1.ptau"))
    hb = _ok("powersoftau", "beacon", "--name", "beacon", path("f1.ptau"), path("fb.ptau"), HASH.hex().upper(), str(EXP)).strip()
    fb = (tmp_path / "fb.ptau").read_bytes()
    want, digest = PKG.ptau_beacon((tmp_path / "f1.ptau").read_bytes(), HASH, EXP, name="beacon")
    assert fb == want and hb == digest.hex()
    out = _ok("powersoftau", "verify", "--require-beacon", path("fb.ptau"))
    assert out.splitlines()[0] == "OK! power 3, 2 contributions" and out.splitlines()[-1] == hb
    _ok("groth16-setup", "--ptau", path("fb.ptau"), "--delta", path("one.txt"), path("c.r1cs"), path("k0.zkey"))
    _ok("groth16-contribute", "--name", "first", "--delta", path("d.txt"), path("k0.zkey"), path("k1.zkey"))
    hk = _ok("groth16-contribute", "--beacon", "--name", "beacon", path("k1.zkey"), path("k2.zkey"), HASH.hex(), str(EXP)).strip()
    k2 = (tmp_path / "k2.zkey").read_bytes()
    assert (k2, bytes.fromhex(hk)) == PKG.groth16_beacon((tmp_path / "k1.zkey").read_bytes(), HASH, EXP, name="beacon")
    out = _ok("groth16-contribute", "--verify-key", "--require-beacon", path("c.r1cs"), path("fb.ptau"), path("k2.zkey"))
    assert out.startswith("OK! ") and out.splitlines()[-1] == hk
    assert "OK! 2 contributions" in _ok("groth16-contribute", "--verify", "--require-beacon", path("k2.zkey"))
    _ok("groth16-setup", "--export-vk", path("k2.zkey"), path("vk.json"))
    assert json.loads((tmp_path / "vk.json").read_text()) == PKG.Groth16VerifyingKey.from_zkey(k2).to_json()
    _ok("groth16-prove", path("c.r1cs"), path("k2.zkey"), path("w.wtns"), path("proof.json"), path("public.json"))
    assert "OK!" in _ok("groth16-verify", path("vk.json"), path("public.json"), path("proof.json"))


def test_cli_require_beacon_refuses_files_that_end_on_a_contribution(tmp_path):
    path = lambda name: str(tmp_path / name)  # noqa: E731
    pl, _ = system()
    (f0, _), (f1, _), _, _ = chain1()
    _, (k1, _), _, _ = chain2()
    for name, data in (("f0.ptau", f0), ("f1.ptau", f1), ("k1.zkey", k1), ("pot.ptau", ptau())):
        (tmp_path / name).write_bytes(data)
    (tmp_path / "c.r1cs").write_bytes(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=0, n_pub_in=0))
    for name in ("f0.ptau", "f1.ptau"):
        p = _run("powersoftau", "verify", "--require-beacon", path(name))
        assert (p.returncode, p.stdout, p.stderr) == (1, "", "INVALID: ptau: %s\n" % NOT_A_BEACON), name
    p = _run("groth16-contribute", "--verify", "--require-beacon", path("k1.zkey"))
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "INVALID: zkey: %s\n" % NOT_A_BEACON)
    p = _run("groth16-contribute", "--verify-key", "--require-beacon", path("c.r1cs"), path("pot.ptau"), path("k1.zkey"))
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "INVALID: zkey: %s\n" % NOT_A_BEACON)
    assert _ok("groth16-contribute", "--verify", path("k1.zkey")).startswith("OK! 1 contributions")
