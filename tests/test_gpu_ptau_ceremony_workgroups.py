"""A powers-of-tau ceremony on an MI355X (r1cs/ceremony.hip) on files of power 8, the smallest whose section 2 has more than 256
points: its 511 points are two workgroups of fr_scalars_kernel with exponents up to 510 (the table entries tau'^(2^b) for
b = 0 .. 8), the 256 points of section 3 four one-wave workgroups of mul_points_kernel, and the whole-file sum of section 3 in
ptau_verify and ptau_verify_step four workgroups (the G1 sums go through the device 256 points at a time at this power, and
section 2's in two ranges).  tests/test_gpu_ptau_ceremony.py and tests/test_gpu_beacon.py run at powers 3
and 4, where a section has 31 points at the most; the helpers here restate theirs.  The oracle is the same: a file written from
the logs holds after a contribution exactly the bytes of the file written from the products.  The Python curve is too slow for
these sizes, so the points of the expected files come from the fixed-base table kernel (bn254_gen_mul_batch_device); every
comparison is byte equality.

Wall time of each test on an MI355X, in seconds (the module's fixtures are built by the first test that needs them):
  test_a_contribution_gives_the_file_of_the_products 0.04         test_a_contribution_in_pieces 0.07 (100), 0.03 (257)
  test_two_contributions_from_a_new_file 0.06                     test_the_honest_chain_is_accepted 0.18
  test_a_beacon_closes_the_chain 0.41                             test_the_whole_file_check_reads_the_points_past_the_first_workgroup 0.43
  test_a_point_fault_has_its_index_in_the_section_whatever_the_piece 0.07
"""
import ctypes
import functools
import math
import random
import struct

import numpy as np
import pytest

import cwc_import
from tests import beacon_fixtures as BF
from tests import ceremony_fixtures as CE
from tests import contribution_fixtures as CF
from tests import groth16_fixtures as GF
from tests import ptau_fixtures as PF

PKG = cwc_import.load()
R, Q = GF.R, GF.Q
POWER, EXP = 8, 10
N = 1 << POWER
SEED = bytes(range(13, 45))
HASH = bytes.fromhex("00000000000000000001a1b2c3d4e5f60718293a4b5c6d7e8f90a1b2c3d4e5f6")  # the shape of a block hash
_rnd = random.Random(1400)
TAU, ALPHA, BETA = (_rnd.randrange(2, R) for _ in range(3))
FIRST, SECOND = (tuple(_rnd.randrange(2, R) for _ in range(3)) for _ in range(2))
OFF_CURVE_Y = GF.lem(1)
CONSECUTIVE = {2: "ptau: section 2 (tauG1): the points are not consecutive powers of the tau of section 3",
               3: "ptau: section 3 (tauG2): the points are not the powers of the tau of section 2",
               4: "ptau: section 4 (alphaTauG1): the points are not alphaTauG1[0] times the powers of tau",
               5: "ptau: section 5 (betaTauG1): the points are not betaTauG1[0] times the powers of tau"}

pytestmark = pytest.mark.gpu


# -- helpers of tests/test_gpu_ptau_ceremony.py and tests/test_gpu_beacon.py, restated -----------------------------------------------
def device_points(group, scalars):
    """[k] -> the stored form of k G, through bn254_gen_mul_batch_device (existing code)"""
    import torch
    arr = np.frombuffer(b"".join((k % R).to_bytes(32, "little") for k in scalars), dtype=np.uint8).reshape(len(scalars), 32)
    out = PKG.bn254_gen_mul_batch_device(torch.from_numpy(arr.copy()).cuda(), group)
    torch.cuda.synchronize()
    raw = out.cpu().numpy().tobytes()
    return b"".join(GF.lem(int.from_bytes(raw[o:o + 32], "little")) for o in range(0, len(raw), 32))


def split(image):
    """[(id, body)] of a binfile in file order"""
    (n,), off, out = struct.unpack_from("<I", image, 8), 12, []
    for _ in range(n):
        sid, size = struct.unpack_from("<IQ", image, off)
        out.append((sid, image[off + 12:off + 12 + size]))
        off += 12 + size
    assert off == len(image)
    return out


def join(sections):
    return b"ptau" + struct.pack("<II", 1, len(sections)) + b"".join(GF.section(i, b) for i, b in sections)


def with_section(image, sid, body):
    return join([(i, body if i == sid else b) for i, b in split(image)])


def with_point(image, sid, index, stored):
    """`image` with the point `index` of section sid replaced"""
    body = dict(split(image))[sid]
    return with_section(image, sid, body[:len(stored) * index] + stored + body[len(stored) * (index + 1):])


def products(*triples):
    return tuple(math.prod(t[j] for t in triples) % R for j in range(3))


@functools.lru_cache(maxsize=None)
def sections_of(logs):
    """sections 1 to 7 of the file of power 8 written from the logs (tau, alpha, beta)"""
    return PF.sections(POWER, *logs, points=device_points)


@functools.lru_cache(maxsize=None)
def written():
    """the input of the single contributions: the file of (TAU, ALPHA, BETA)"""
    return PF.assemble(sections_of((TAU, ALPHA, BETA)))


@functools.lru_cache(maxsize=None)
def chain():
    """ptau_new and two contributions: [(file, digest)]"""
    f0 = PKG.ptau_new(POWER)
    f1, d1 = PKG.ptau_contribute(f0, name="first", secrets=FIRST)
    f2, d2 = PKG.ptau_contribute(f1, name="second", secrets=SECOND)
    return (f0, None), (f1, d1), (f2, d2)


def verdict(call, *args):
    """(rc, message) of gwb_ptau_verify or gwb_ptau_verify_step through the C ABI"""
    st = PKG.GwStatus()
    rc = call(*args, ctypes.byref(st))
    msg = ctypes.string_at(st.error_msg).decode() if st.error_msg else ""
    return rc, msg


def verify_rc(image, flags=0):
    n = ctypes.c_size_t(0)
    return verdict(PKG.r1cs_lib().gwb_ptau_verify, image, len(image), flags, SEED, None, ctypes.byref(n))


def step_rc(prev, nxt):
    return verdict(PKG.r1cs_lib().gwb_ptau_verify_step, prev, len(prev), nxt, len(nxt), SEED)


def assert_sections(image, logs):
    """sections 1 to 6 of `image` are those of the file written from `logs`"""
    want = sections_of(logs)
    got = split(image)
    assert [i for i, _ in got] == [1, 2, 3, 4, 5, 6, 7]
    for sid, body in got[:6]:
        assert body == want[sid], "section %d differs" % sid


# -- 1. the contribution's bytes ----------------------------------------------------------------------------------------------------
def test_a_contribution_gives_the_file_of_the_products():
    out, digest = PKG.ptau_contribute(written(), secrets=FIRST)
    assert_sections(out, products((TAU, ALPHA, BETA), FIRST))
    assert PKG.ptau_info(out) == {"power": POWER, "ceremony_power": POWER, "prepared": False, "n_contributions": 1}
    assert PKG.ptau_contributions(out)[0]["next_challenge"] == digest


@pytest.mark.parametrize("chunk", (100, 257))
def test_a_contribution_in_pieces(chunk, monkeypatch):
    """pieces of 100 points begin at the exponents 100, 200, ..., end inside every section, and the last one is short; a piece of
    257 points is one point longer than a workgroup of fr_scalars_kernel"""
    monkeypatch.setenv("CWC_CONTRIBUTE_CHUNK", str(chunk))
    out, _ = PKG.ptau_contribute(written(), secrets=FIRST)
    assert_sections(out, products((TAU, ALPHA, BETA), FIRST))


# -- 2. the chain -------------------------------------------------------------------------------------------------------------------
def test_two_contributions_from_a_new_file():
    _, (f1, _), (f2, _) = chain()
    assert_sections(f1, FIRST)
    assert_sections(f2, products(FIRST, SECOND))


def test_the_honest_chain_is_accepted():
    (f0, _), (f1, d1), (f2, d2) = chain()
    assert PKG.ptau_verify(f1, seed=SEED) == [d1] and PKG.ptau_verify(f2, seed=SEED) == [d1, d2]
    PKG.ptau_verify_step(f0, f1, seed=SEED)
    PKG.ptau_verify_step(f1, f2, seed=SEED)


def test_a_beacon_closes_the_chain():
    """expected_ptau of tests/test_gpu_beacon.py at power 8: sections 1 to 6 of the writer for the products with the beacon's
    scalars, section 7 = the earlier records and the fixture's beacon"""
    (_, _), (_, d1), (f2, d2) = chain()
    fb, db = PKG.ptau_beacon(f2, HASH, EXP, name="beacon")
    logs = products(FIRST, SECOND)
    secs = dict(split(f2))
    want = sections_of(products(logs, BF.scalars(1, HASH, EXP)[:3]))
    earlier = CE.read_section7(secs[7])
    rec = BF.ptau_beacon_record(earlier[-1].next_challenge, logs, HASH, EXP, "beacon")
    assert rec.type == 1 and rec.params == CF.beacon_params("beacon", EXP, HASH)
    body7 = struct.pack("<I", 3) + secs[7][4:] + rec.stored()
    assert fb == join([(1, secs[1])] + [(sid, want[sid]) for sid in range(2, 7)] + [(7, body7)]) and db == rec.next_challenge
    assert PKG.ptau_verify(fb, seed=SEED, require_beacon=True) == [d1, d2, db]


# -- 3. the whole-file check beyond the first workgroup -----------------------------------------------------------------------------
def test_the_whole_file_check_reads_the_points_past_the_first_workgroup():
    """one foreign point of the subgroup per section, in the whole-file sums of ptau_verify and of ptau_verify_step: tauG1[300] in
    the second range of section 2's sum (the points 256 .. 509), tauG2[200] in the fourth one-wave workgroup of section 3's.
    Sections 4 and 5 have 256 points at this power: alphaTauG1[255] (the section's last point; it has no point 257) and
    betaTauG1[129]."""
    (f0, _), (f1, _), _ = chain()
    foreign1, foreign2 = device_points(1, [12345]), device_points(2, [12345])
    for sid, index, foreign in ((2, 300, foreign1), (3, 200, foreign2), (4, 255, foreign1), (5, 129, foreign1)):
        bad = with_point(f1, sid, index, foreign)
        assert verify_rc(bad) == (1, CONSECUTIVE[sid]), (sid, index)
        assert step_rc(f0, bad) == (1, CONSECUTIVE[sid]), (sid, index)
    PKG.ptau_check_powers(with_point(f1, 2, 300, foreign1), 7, seed=SEED)  # the prefix of 2 * 2^7 points ends before the point 300


# -- 4. fault indices across pieces -------------------------------------------------------------------------------------------------
def off_curve(image, sid, index):
    """the y (in G2 its first component) of the point `index` of section sid replaced by 1"""
    width = 128 if sid == 3 else 64
    body = dict(split(image))[sid]
    at = width * index + width // 2
    return with_section(image, sid, body[:at] + OFF_CURVE_Y + body[at + 32:])


def test_a_point_fault_has_its_index_in_the_section_whatever_the_piece(monkeypatch):
    """pieces of 100 points: the flag holds an index in the piece (42 of the fourth piece, 30 of the second), the message the index
    in the section.  Two faults in one section: the earlier piece ends the call (150 before 342), and inside one piece, in two
    waves of it, the flag's atomicMin keeps the smaller index (310 before 399)."""
    monkeypatch.setenv("CWC_CONTRIBUTE_CHUNK", "100")
    with pytest.raises(PKG.WitnessCalcError, match=r"^ptau: section 2 \(tauG1\) point 342 is not on the G1 curve$"):
        PKG.ptau_contribute(off_curve(written(), 2, 342), secrets=FIRST)
    body = sections_of((TAU, ALPHA, BETA))[3]
    big = with_section(written(), 3, body[:128 * 130] + Q.to_bytes(32, "little") + body[128 * 130 + 32:])
    with pytest.raises(PKG.WitnessCalcError, match=r"^ptau: section 3 \(tauG2\) point 130 has a coordinate >= q$"):
        PKG.ptau_contribute(big, secrets=FIRST)
    with pytest.raises(PKG.WitnessCalcError, match=r"^ptau: section 2 \(tauG1\) point 150 is not on the G1 curve$"):
        PKG.ptau_contribute(off_curve(off_curve(written(), 2, 342), 2, 150), secrets=FIRST)
    with pytest.raises(PKG.WitnessCalcError, match=r"^ptau: section 2 \(tauG1\) point 310 is not on the G1 curve$"):
        PKG.ptau_contribute(off_curve(off_curve(written(), 2, 399), 2, 310), secrets=FIRST)
