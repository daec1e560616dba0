"""The host side of the phase-2 contributions (r1cs/contributions.cc, include/graph_witness_groth16_contribute.h): BLAKE2b-512
against hashlib, the challenge point against tests/contribution_fixtures.py, section 10 read from Python-written bytes, every
refusal of its reader, and the CLI's exits that need no device."""
import ctypes
import hashlib
import os
import random
import struct
import subprocess

import pytest

import cwc_import
from tests import contribution_fixtures as CF
from tests import g2_subgroup_fixtures as SF
from tests import groth16_fixtures as GF

PKG = cwc_import.load()
R, Q = GF.R, GF.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "circom-witnesscalc_amd", "groth16-contribute")


@pytest.mark.parametrize("n", (0, 1, 127, 128, 129, 255, 256, 1000))
def test_blake2b512(n):
    data = bytes(random.Random(n).randrange(256) for _ in range(n))
    out = ctypes.create_string_buffer(64)
    PKG.r1cs_lib().gwb_blake2b512(data, n, out)
    assert out.raw == hashlib.blake2b(data).digest()


def _challenge(t):
    out = ctypes.create_string_buffer(128)
    PKG.r1cs_lib().gwb_zkey_contribution_challenge(t, out)
    return out.raw


def _transcripts():
    """16 transcripts: 12 seeded ones and 4 found by search whose counter 0 is rejected, two for a coordinate >= q and two for
    a right-hand side that is no square"""
    rnd = random.Random(2025)
    out = [bytes(rnd.randrange(256) for _ in range(64)) for _ in range(12)]
    want = {"range": 2, "square": 2}
    while any(want.values()):
        t = bytes(rnd.randrange(256) for _ in range(64))
        d = CF.H(t + b"cwc-g2" + struct.pack("<I", 0))
        c0, c1 = (int.from_bytes(h, "little") & ((1 << 254) - 1) for h in (d[:32], d[32:]))
        if c0 >= Q or c1 >= Q:
            kind = "range"
        else:
            x = (c0, c1)
            rhs = GF.Fq2.add(GF.Fq2.mul(GF.Fq2.mul(x, x), x), GF.B2)
            kind = "square" if pow((rhs[0] * rhs[0] + rhs[1] * rhs[1]) % Q, (Q - 1) // 2, Q) != 1 else None
        if kind and want[kind]:
            want[kind] -= 1
            out.append(t)
    return out


def test_hash_to_g2():
    ts = _transcripts()
    assert len(ts) == 16
    first_reasons = []
    for t in ts:
        p, why = CF.hash_to_g2_trace(t)
        first_reasons.append(why[0] if why else None)
        assert GF.G2.on_curve(p) and SF.in_g2_by_order(p)
        assert _challenge(t) == CF.canonical_g2(p), "transcript %s" % t.hex()
    assert first_reasons[12:].count("range") == 2 and first_reasons[12:].count("square") == 2


# -- section 10 -----------------------------------------------------------------------------------------------------------------
def _key_with(sec10):
    """the smallest file zkey_contributions reads: the section table and section 10"""
    return b"zkey" + struct.pack("<II", 1, 1) + GF.section(10, sec10)


def _records(n, beacon_at=None):
    rnd = random.Random(77 + n)
    cs_hash = bytes(rnd.randrange(256) for _ in range(64))
    recs, delta_prev = [], GF.G1.gen
    for k in range(n):
        rec = CF.contribution(cs_hash, recs, delta_prev, rnd.randrange(1, R), rnd.randrange(1, R), name="party %d" % k if k != 1 else "")
        if k == beacon_at:
            rec.type = 1
            rec.params = CF.beacon_params("beacon", 10, bytes(range(32)))
        recs.append(rec)
        delta_prev = rec.delta_after
    return cs_hash, recs


@pytest.mark.parametrize("n,beacon_at", ((0, None), (1, None), (3, 2)))
def test_zkey_contributions(n, beacon_at):
    cs_hash, recs = _records(n, beacon_at)
    body = CF.write_section10(cs_hash, recs)
    got = PKG.zkey_contributions(_key_with(body))
    assert got["cs_hash"] == cs_hash and len(got["contributions"]) == n
    for k, (g, r) in enumerate(zip(got["contributions"], recs)):
        assert g["type"] == (1 if k == beacon_at else 0)
        assert g["name"] == ("beacon" if k == beacon_at else "" if k == 1 else "party %d" % k)
        assert g["delta_after"] == CF.canonical_g1(r.delta_after) and g["g1_s"] == CF.canonical_g1(r.g1_s)
        assert g["g1_sx"] == CF.canonical_g1(r.g1_sx) and g["g2_spx"] == CF.canonical_g2(r.g2_spx)
        assert g["transcript"] == r.transcript and g["hash"] == r.hash()
    # the Python reader agrees with the Python writer
    back_hash, back = CF.read_section10(body)
    assert back_hash == cs_hash and [r.stored() for r in back] == [r.stored() for r in recs]


def _refused(body, pattern):
    with pytest.raises(PKG.WitnessCalcError, match=r"^zkey: section 10 .*" + pattern):
        PKG.zkey_contributions(_key_with(body))


def test_section10_refusals():
    cs_hash, recs = _records(2)
    good = CF.write_section10(cs_hash, recs)
    first_len = len(recs[0].stored())
    PKG.zkey_contributions(_key_with(good))
    # truncated
    _refused(b"", "truncated")
    _refused(good[:67], "truncated")
    _refused(good[:68 + first_len + 100], "declares 2 contributions")
    assert first_len > 392
    _refused(good[:68 + 2 * 392], "contribution 2: the record is truncated")
    # a count the section cannot hold
    _refused(good[:64] + struct.pack("<I", 3) + good[68:], "declares 3 contributions")
    _refused(good[:64] + struct.pack("<I", 0xffffffff) + good[68:], "declares 4294967295 contributions")
    _refused(good[:64] + struct.pack("<I", 1) + good[68:], "trailing bytes")
    # paramsLen past the end
    at = 68 + 388
    _refused(good[:at] + struct.pack("<I", 100000) + good[at + 4:], "contribution 1: paramsLen 100000 runs past the section's end")
    last = 68 + first_len + 388
    _refused(good[:last] + struct.pack("<I", len(recs[1].params) + 1) + good[last + 4:], "contribution 2: paramsLen")
    # an item length past the parameters' end, a cut item 02, an unknown tag
    def with_params(params):
        r = CF.Record(recs[0].delta_after, recs[0].g1_s, recs[0].g1_sx, recs[0].g2_spx, recs[0].transcript, 0, params)
        return CF.write_section10(cs_hash, [r])
    PKG.zkey_contributions(_key_with(with_params(bytes([1, 3]) + b"abc" + bytes([2, 9, 3, 2, 7, 7]))))
    _refused(with_params(bytes([1, 4]) + b"abc"), "contribution 1: the length of parameter 01 runs past")
    _refused(with_params(bytes([1])), "the length of parameter 01 runs past")
    _refused(with_params(bytes([3, 33]) + bytes(32)), "the length of parameter 03 runs past")
    _refused(with_params(bytes([2])), "parameter 02 .* runs past")
    _refused(with_params(bytes([4, 0])), "contribution 1: unknown parameter tag 4")
    _refused(with_params(bytes([0])), "unknown parameter tag 0")
    # an unknown type
    at = 68 + 384
    _refused(good[:at] + struct.pack("<I", 2) + good[at + 4:], "contribution 1: unknown type 2")
    # points: a coordinate >= q in every slot, a point off its curve
    for name, off, words in (("deltaAfter", 0, 2), ("g1_s", 64, 2), ("g1_sx", 128, 2), ("g2_spx", 192, 4)):
        for w in range(words):
            at = 68 + off + 32 * w
            _refused(good[:at] + Q.to_bytes(32, "little") + good[at + 32:], "contribution 1: %s has a coordinate >= q" % name)
        at = 68 + off
        bad = GF.lem(1) + GF.lem(3) if words == 2 else GF.lem(1) + GF.lem(0) + GF.lem(1) + GF.lem(0)
        _refused(good[:at] + bad + good[at + 32 * words:], "contribution 1: %s is not on the G%d curve" % (name, words // 2))
    at = 68 + first_len + 64
    _refused(good[:at] + GF.lem(1) + GF.lem(3) + good[at + 64:], "contribution 2: g1_s is not on the G1 curve")


def test_missing_section10():
    with pytest.raises(PKG.WitnessCalcError, match="zkey: section 10 is missing"):
        PKG.zkey_contributions(b"zkey" + struct.pack("<II", 1, 1) + GF.section(1, struct.pack("<I", 1)))


# -- the CLI, without a device ----------------------------------------------------------------------------------------------------
def test_cli_exits(tmp_path):
    path = lambda name: str(tmp_path / name)  # noqa: E731
    p = subprocess.run([CLI, path("none.zkey"), path("out.zkey")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "cannot read" in p.stderr
    p = subprocess.run([CLI, "--verify", path("none.zkey")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "cannot read" in p.stderr
    p = subprocess.run([CLI, "--verify-step", path("none.zkey"), path("other.zkey")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "cannot read" in p.stderr
    (tmp_path / "in.zkey").write_bytes(_key_with(CF.NO_RECORDS))
    for text in ("12x\n", "", "1 2\n", "1" + "0" * 78 + "\n"):
        (tmp_path / "d.txt").write_text(text)
        p = subprocess.run([CLI, "--delta", path("d.txt"), path("in.zkey"), path("out.zkey")], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "delta" in p.stderr and not (tmp_path / "out.zkey").exists(), (text, p)
    p = subprocess.run([CLI, "--delta", path("missing.txt"), path("in.zkey"), path("out.zkey")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "cannot read" in p.stderr
    # a file that is no key: refused by the loader, before any device work
    (tmp_path / "d.txt").write_text("5\n")
    p = subprocess.run([CLI, "--delta", path("d.txt"), path("in.zkey"), path("out.zkey")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "zkey: missing section" in p.stderr and not (tmp_path / "out.zkey").exists()
    p = subprocess.run([CLI], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "usage" in p.stderr
