"""ptau_prepare_phase2 and ptau_check_lagrange on an MI355X at power 9, the smallest file whose all-level launches all have more
than one workgroup of 256 threads: the top levels are 9 and 10, so a stage launch of idft_levels_stage_kernel (setup_ptau.hip),
fr_levels_stage_kernel and fold_levels_kernel (contribute.hip) has 2 or 4 workgroups, the wave-uniform stages reach s = 3 and
s = 4 (twiddle indices up to 15), and scale_levels_kernel and rho_levels_kernel run 4 and 8 workgroups over the 1023 and 2047
slots.  tests/test_gpu_ptau_prepare.py stops at power 7, where every such launch is one workgroup; the helpers here restate its
own.  Expected points are scalars times the generator, the scalars from the closed forms of tests/ptau_fixtures.py and the
points from the fixed-base table kernel (bn254_gen_mul_batch_device); affine stored points are unique, so every comparison is
byte equality.  The faults lie past the first 256 points of their level, array or section.

Wall time of each test on an MI355X, in seconds (the module's fixtures are built by the first test that needs them; the 24 tests
of this module and the 8 of tests/test_gpu_ptau_ceremony_workgroups.py together: 8.2):
  test_prepared_bytes 1.83 (the honest file, its prepared form and the expected sections)
  test_prepared_and_checked_in_pieces_of_300_points 0.38          test_check_accepts_every_level_at_once 0.15
  test_check_accepts_one_domain 0.05, 0.06                        test_check_refuses_a_foreign_monomial_point 0.12
  test_check_refuses_a_fault_past_the_first_workgroup 0.14 to 0.18 in G1, 0.31 in section 13 (15 cases)
  test_check_names_a_point_fault_past_slot_512 < 0.01 (refused on the host)
  test_prepare_names_a_point_fault_past_the_first_workgroup 0.19  test_prepared_file_feeds_the_setup 0.69
"""
import functools
import random
import struct

import numpy as np
import pytest

import cwc_import
from tests import groth16_fixtures as GF
from tests import ptau_fixtures as PF
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
R, Q = GF.R, GF.Q
MONT_INV = pow(GF.MONT, -1, Q)
SEED = bytes(range(11, 43))
POWER = 9
N = 1 << POWER
WIDTH = {12: 64, 13: 128, 14: 64, 15: 64}
NAME = {12: "lagrange tauG1", 13: "lagrange tauG2", 14: "lagrange alphaTauG1", 15: "lagrange betaTauG1"}
OFF_CURVE_G1 = GF.lem(1) + GF.lem(3)

_rnd = random.Random(1300)
TAU, ALPHA, BETA, TAU_OTHER, DELTA_RANDOM = (_rnd.randrange(2, R) for _ in range(5))

pytestmark = pytest.mark.gpu


# -- helpers of tests/test_gpu_ptau_prepare.py, restated ------------------------------------------------------------------------
def device_canonical(group, scalars):
    """[k] -> uint8 [n, 64 group]: k G, canonical affine, zero bytes for infinity"""
    import torch
    arr = np.frombuffer(b"".join((k % R).to_bytes(32, "little") for k in scalars), dtype=np.uint8).reshape(len(scalars), 32)
    out = PKG.bn254_gen_mul_batch_device(torch.from_numpy(arr.copy()).cuda(), group)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def device_points(group, scalars):
    """ptau_fixtures' `points`: the stored form (Montgomery little-endian) of k G"""
    raw = device_canonical(group, scalars).tobytes()
    return b"".join(GF.lem(int.from_bytes(raw[o:o + 32], "little")) for o in range(0, len(raw), 32))


@functools.lru_cache(maxsize=None)
def file_sections(prepared=False, lagrange_tau=None):
    return PF.sections(POWER, TAU, ALPHA, BETA, prepared=prepared, lagrange_tau=lagrange_tau, points=device_points)


@functools.lru_cache(maxsize=None)
def plain():
    return PF.assemble(file_sections())


@functools.lru_cache(maxsize=None)
def prepared():
    """the library's own output for the honest file"""
    return PKG.ptau_prepare_phase2(plain())


@functools.lru_cache(maxsize=None)
def truncated_top():
    """level POWER + 1 of section 12 as the library defines it: Lag of (T_0 .. T_{2n-2}, O)"""
    t = [pow(TAU, i, R) for i in range(2 * N - 1)]
    return device_points(1, PF.lag(POWER + 1, t + [0]))


def split(image):
    """`.ptau` bytes -> [(id, body)] in file order"""
    assert image[:4] == b"ptau" and struct.unpack_from("<I", image, 4)[0] == 1
    off, out = 12, []
    for _ in range(struct.unpack_from("<I", image, 8)[0]):
        sid, size = struct.unpack_from("<IQ", image, off)
        out.append((sid, image[off + 12:off + 12 + size]))
        off += 12 + size
    assert off == len(image)
    return out


def with_section(image, sid, body):
    """`image` with the body of one section replaced"""
    secs = dict(split(image))
    secs[sid] = body
    return PF.assemble(secs)


def _fq(b):
    return int.from_bytes(b, "little") * MONT_INV % Q


def point_of(stored):
    c = [_fq(stored[o:o + 32]) for o in range(0, len(stored), 32)]
    return (c[0], c[1]) if len(c) == 2 else ((c[0], c[1]), (c[2], c[3]))


def stored_of(curve, jac):
    return (GF.g1_bytes if curve is GF.G1 else GF.g2_bytes)(curve.to_affine(jac))


def system(p):
    """the planted system of test_gpu_groth16_setup.py::power_case for the domain 2^p (construction restated): its R1cs"""
    n_pub_in, n_pub = 2, 3
    n_c = (1 << p) - n_pub - 1 - random.Random(p).randrange(0, 1 << (p - 1))
    rnd = random.Random(100 + p)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(n_c)]
    pl = F.planted_system(rnd, 6, shapes, [1, R - 1, 2, F.MONT_R, None])
    r1 = PKG.R1cs(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=n_pub - n_pub_in, n_pub_in=n_pub_in))
    assert r1.qap_info()["domain_power"] == p
    return r1


@functools.lru_cache(maxsize=None)
def level_faults(sid, m, k):
    """{name: the prepared file with that fault in level m of section sid}, level_faults of test_gpu_ptau_prepare.py with the fault
    at the offset k of the level and not at its end: the point k doubled, the points k - 1 and k swapped, and the points from k to
    the level's end taken from the file of another tau (the level's first k points stay honest)"""
    width, body, first = WIDTH[sid], dict(split(prepared()))[sid], (1 << m) - 1
    assert 256 <= k < (1 << m) - 1
    curve = GF.G2 if sid == 13 else GF.G1
    at = lambda j: width * (first + j)  # noqa: E731
    put = lambda j, new: with_section(prepared(), sid, body[:at(j)] + new + body[at(j) + len(new):])  # noqa: E731
    here = body[at(k):at(k) + width]
    other = file_sections(True, TAU_OTHER)[sid][at(k):at(1 << m)]
    assert other != body[at(k):at(1 << m)] and here != body[at(k - 1):at(k)]
    return {"doubled": put(k, stored_of(curve, curve.mul(point_of(here), 2))),
            "swapped": put(k - 1, here + body[at(k - 1):at(k)]),
            "another_tau": put(k, other)}


# -- 1. the bytes ---------------------------------------------------------------------------------------------------------------
def test_prepared_bytes():
    """sections 13, 14 and 15 and section 12 below its last level against the fixture, the last level of section 12 against the
    truncated definition (the fixture writes it from the true tau), the sections before them carried"""
    out = prepared()
    got, want = dict(split(out)[-4:]), file_sections(True)
    assert [sid for sid, _ in split(out)[-4:]] == [12, 13, 14, 15]
    for sid in (13, 14, 15):
        assert got[sid] == want[sid], "section %d differs" % sid
    shared = 64 * (2 * N - 1)
    assert len(got[12]) == 64 * (4 * N - 1)
    assert got[12][:shared] == want[12][:shared], "section 12 differs below its last level"
    assert got[12][shared:] == truncated_top(), "the last level of section 12 is not Lag of (T_0 .. T_{2n-2}, O)"
    assert split(out)[:-4] == split(plain())
    info = PKG.ptau_info(out)
    assert info["prepared"] and info["power"] == POWER


def test_prepared_and_checked_in_pieces_of_300_points(monkeypatch):
    """300 divides neither the levels nor the workgroups, and the last piece of every section is short"""
    monkeypatch.setenv("CWC_CONTRIBUTE_CHUNK", "300")
    assert PKG.ptau_prepare_phase2(plain()) == prepared()
    PKG.ptau_check_lagrange(prepared(), seed=SEED)


# -- 2. the check accepts -------------------------------------------------------------------------------------------------------
def test_check_accepts_every_level_at_once():
    for seed in (SEED, bytes(32), None):
        PKG.ptau_check_lagrange(prepared(), seed=seed)


@pytest.mark.parametrize("p", (7, 8))
def test_check_accepts_one_domain(p):
    """domain 8 reads the levels 8 and 9 of section 12: fr_levels_stage_kernel with m_lo = m_hi = 9 on two workgroups, every
    lower level filtered out"""
    PKG.ptau_check_lagrange(prepared(), p, seed=SEED)


# -- 3. the check refuses beyond the first workgroup ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("doubled", "swapped", "another_tau"))
@pytest.mark.parametrize("sid,m,k", [(12, 9, 300), (12, 10, 700), (13, 9, 257), (14, 9, 301), (15, 9, 417)])
def test_check_refuses_a_fault_past_the_first_workgroup(sid, m, k, name):
    """all-level mode names the section and finds the level; the domain that reads the level (8 for level 9 of section 12, none
    for the last level of a section) names section and level; a domain that does not read it accepts the file"""
    file = level_faults(sid, m, k)[name]
    who = r"^ptau: section %d \(%s\)" % (sid, NAME[sid])
    says = " does not hold the Lagrange forms of section %d" % (sid - 10)
    with pytest.raises(PKG.WitnessCalcError, match=who + says + ": level %d is the first that does not$" % m):
        PKG.ptau_check_lagrange(file, seed=SEED)
    if sid == 12 and m == POWER:
        with pytest.raises(PKG.WitnessCalcError, match=who + " level %d" % m + says + "$"):
            PKG.ptau_check_lagrange(file, POWER - 1, seed=SEED)
    PKG.ptau_check_lagrange(file, 7, seed=SEED)  # the bystander: levels 7 and 8 only


def test_check_refuses_a_foreign_monomial_point():
    """alpha T_300 replaced by another point of the subgroup: of section 14, level 9 alone sums it"""
    body = file_sections()[4]
    file = with_section(prepared(), 4, body[:64 * 300] + device_points(1, [12345]) + body[64 * 301:])
    with pytest.raises(PKG.WitnessCalcError, match=r"^ptau: section 14 \(lagrange alphaTauG1\) does not hold the Lagrange forms of section 4: "
                                                   r"level 9 is the first that does not$"):
        PKG.ptau_check_lagrange(file, seed=SEED)


def test_check_names_a_point_fault_past_slot_512():
    body = dict(split(prepared()))
    bad = with_section(prepared(), 14, body[14][:64 * 600] + OFF_CURVE_G1 + body[14][64 * 601:])
    with pytest.raises(PKG.WitnessCalcError, match=r"^ptau: section 14 \(lagrange alphaTauG1\) point 600 is not on the G1 curve"):
        PKG.ptau_check_lagrange(bad, seed=SEED)
    at = 128 * 700
    bad = with_section(prepared(), 13, body[13][:at + 96] + Q.to_bytes(32, "little") + body[13][at + 128:])
    with pytest.raises(PKG.WitnessCalcError, match=r"^ptau: section 13 \(lagrange tauG2\) point 700 has a coordinate >= q"):
        PKG.ptau_check_lagrange(bad, seed=SEED)


# -- 4. prepare names a fault ---------------------------------------------------------------------------------------------------
def test_prepare_names_a_point_fault_past_the_first_workgroup():
    secs = file_sections()
    for sid, width, index, fault, pattern in ((2, 64, 400, OFF_CURVE_G1, r"section 2 \(tauG1\) point 400 is not on the G1 curve"),
                                              (3, 128, 300, bytes(32) + Q.to_bytes(32, "little") + bytes(64), r"section 3 \(tauG2\) point 300 has a coordinate >= q")):
        bad = dict(secs)
        bad[sid] = secs[sid][:width * index] + fault + secs[sid][width * (index + 1):]
        with pytest.raises(PKG.WitnessCalcError, match=pattern):
            PKG.ptau_prepare_phase2(PF.assemble(bad))


# -- 5. it feeds the setup ------------------------------------------------------------------------------------------------------
def test_prepared_file_feeds_the_setup():
    """the domain 2^8 reads level 8 of the four sections and the odd points of level 9 of section 12, as the device wrote them: the
    key read from the prepared file is the key computed from the plain one"""
    r1 = system(8)
    assert PKG.groth16_setup_ptau(r1, prepared(), DELTA_RANDOM, "file") == PKG.groth16_setup_ptau(r1, plain(), DELTA_RANDOM, "compute")
