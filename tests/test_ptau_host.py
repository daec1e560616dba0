"""The `.ptau` loader's host side (r1cs/ptau.cc, include/graph_witness_groth16_ptau.h) on files written by tests/ptau_fixtures.py:
ptau_info, every refusal with its message, unknown sections and sections out of order.  gwb_ptau_info and gwb_ptau_check do not
touch a device, and gwb_groth16_setup_ptau refuses a file, a domain and a delta before it does, so all of this holds on a machine
without one; the groth16-setup CLI's exit status 2 for --ptau usage and file errors."""
import functools
import mmap
import os
import random
import struct
import subprocess

import pytest

import cwc_import
from tests import groth16_fixtures as GF
from tests import ptau_fixtures as PF
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
R, Q = F.R, GF.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "circom-witnesscalc_amd", "groth16-setup")
TAU, ALPHA, BETA = 0x1234567, 0x89abcd, 0xfedcba9
POWER = 3


@functools.lru_cache(maxsize=None)
def secs(prepared=False):
    return PF.sections(POWER, TAU, ALPHA, BETA, prepared=prepared, n_contributions=5, ceremony_power=12)


def broken(prepared=False, **changes):
    """the file with the bodies of the given sections (s2=..., s13=...) replaced"""
    s = dict(secs(prepared))
    for k, v in changes.items():
        s[int(k[1:])] = v
    return PF.assemble(s)


def patched(body, at, new):
    return body[:at] + new + body[at + len(new):]


def refuses(data, pattern, p=2, lagrange="auto"):
    with pytest.raises(PKG.WitnessCalcError, match=pattern):
        PKG.ptau_check(data, p, lagrange)


def test_info_plain_and_prepared():
    want = {"power": POWER, "ceremony_power": 12, "prepared": False, "n_contributions": 5}
    assert PKG.ptau_info(PF.assemble(secs())) == want
    assert PKG.ptau_info(PF.assemble(secs(True))) == dict(want, prepared=True)
    for p in (1, 2):
        for mode in ("auto", "compute"):
            PKG.ptau_check(PF.assemble(secs()), p, mode)
        for mode in ("auto", "file", "compute"):
            PKG.ptau_check(PF.assemble(secs(True)), p, mode)
    # one prepared section of another size: the file counts as not prepared
    s = dict(secs(True))
    s[14] = s[14][:-64]
    assert PKG.ptau_info(PF.assemble(s))["prepared"] is False


def test_info_reads_a_mapped_file(tmp_path):
    path = tmp_path / "pot.ptau"
    path.write_bytes(PF.assemble(secs(True)))
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
        assert PKG.ptau_info(m)["prepared"] is True
        PKG.ptau_check(m, 2, "file")


def test_unknown_sections_and_any_order_load():
    s = secs(True)
    data = PF.assemble(s, order=[15, 6, 3, 1, 13, 7, 2, 12, 5, 14, 4], extra=[(8, b"xyz"), (99, bytes(70)), (0, b"")])
    assert PKG.ptau_info(data) == {"power": POWER, "ceremony_power": 12, "prepared": True, "n_contributions": 5}
    PKG.ptau_check(data, 2, "file")
    PKG.ptau_check(data, 2, "compute")
    # no section 7: no contributions stated
    assert PKG.ptau_info(PF.assemble(secs(), order=[1, 2, 3, 4, 5, 6]))["n_contributions"] == 0


def test_container_refusals():
    good = PF.assemble(secs())
    for data, pattern in ((b"ptaw" + good[4:], "bad magic"), (b"pta", "bad magic"), (b"zkey" + good[4:], "bad magic"),
                          (PF.assemble(secs(), version=2), r"unsupported version 2"),
                          (good[:-1], r"truncated section 7"), (good + b"\0", r"1 trailing bytes"),
                          (good[:12] + good[12:20], r"truncated section header")):
        with pytest.raises(PKG.WitnessCalcError, match=pattern):
            PKG.ptau_info(data)


def test_header_refusals():
    h = secs()[1]
    for body, pattern in ((PF.header(POWER, n8=31), r"n8 is not 32"), (PF.header(POWER, n8=48), r"n8 is not 32"),
                          (PF.header(POWER, q=R), r"base field q is not BN254's"), (PF.header(29), r"power 29 is above 28"),
                          (h + b"\0\0\0\0", r"section 1 \(header\) has 48 bytes, 44 expected"), (b"", r"n8 is not 32")):
        with pytest.raises(PKG.WitnessCalcError, match=pattern):
            PKG.ptau_info(broken(s1=body))


@pytest.mark.parametrize("sid", range(1, 7))
def test_missing_required_section(sid):
    with pytest.raises(PKG.WitnessCalcError, match=r"missing section %d \(" % sid):
        PKG.ptau_info(PF.assemble(secs(), order=[i for i in range(1, 8) if i != sid]))


@pytest.mark.parametrize("sid", (1, 2, 6, 13))
def test_duplicate_section(sid):
    with pytest.raises(PKG.WitnessCalcError, match=r"duplicate section %d" % sid):
        PKG.ptau_info(PF.assemble(secs(True), order=sorted(secs(True)) + [sid]))


@pytest.mark.parametrize("sid,unit", ((2, 64), (3, 128), (4, 64), (5, 64), (6, 128)))
def test_missized_required_section(sid, unit):
    body = secs()[sid]
    for b in (body[:-unit], body + bytes(unit), body[:-1]):
        with pytest.raises(PKG.WitnessCalcError, match=r"section %d \(\w+\) has %d bytes, %d expected" % (sid, len(b), len(body))):
            PKG.ptau_info(broken(**{"s%d" % sid: b}))
    # sized for another power than the header states
    with pytest.raises(PKG.WitnessCalcError, match=r"section 2 \(tauG1\) has 960 bytes, 1984 expected"):
        PKG.ptau_info(broken(s1=PF.header(POWER + 1)))


def test_generators_are_required():
    s = secs()
    two_g1 = GF.g1_bytes(GF.G1.gen_muls([2])[0])
    two_g2 = GF.g2_bytes(GF.G2.gen_muls([2])[0])
    with pytest.raises(PKG.WitnessCalcError, match=r"section 2 \(tauG1\) point 0 is not the G1 generator"):
        PKG.ptau_info(broken(s2=patched(s[2], 0, two_g1)))
    with pytest.raises(PKG.WitnessCalcError, match=r"section 3 \(tauG2\) point 0 is not the G2 generator"):
        PKG.ptau_info(broken(s3=patched(s[3], 0, two_g2)))
    with pytest.raises(PKG.WitnessCalcError, match=r"point 0 is not the G1 generator"):
        PKG.ptau_info(broken(s2=patched(s[2], 0, bytes(64))))


Q_BYTES = Q.to_bytes(32, "little")
OFF_G1 = GF.lem(1) + GF.lem(3)                                  # 9 != 1 + 3
OFF_G2 = GF.lem(1) + GF.lem(0) + GF.lem(1) + GF.lem(0)


@pytest.mark.parametrize("sid,unit,index,p", ((2, 64, 7, 2), (2, 64, 1, 1), (3, 128, 3, 2), (4, 64, 0, 2), (4, 64, 3, 2), (5, 64, 0, 1),
                                              (5, 64, 1, 1), (6, 128, 0, 1)))
def test_points_read_are_checked(sid, unit, index, p):
    """a coordinate >= q and a point off its curve at the last index a domain 2^p reads (2n - 1 in tauG1, n - 1 elsewhere),
    at alpha1, beta1 and beta2; the same fault one index further is not read"""
    body, g2 = secs()[sid], unit == 128
    name = {2: "tauG1", 3: "tauG2", 4: "alphaTauG1", 5: "betaTauG1", 6: "betaG2"}[sid]
    for coord in range(unit // 32):
        bad = patched(body, unit * index + 32 * coord, Q_BYTES)
        refuses(broken(**{"s%d" % sid: bad}), r"section %d \(%s\) point %d has a coordinate >= q" % (sid, name, index), p, "compute")
    bad = patched(body, unit * index, OFF_G2 if g2 else OFF_G1)
    refuses(broken(**{"s%d" % sid: bad}), r"section %d \(%s\) point %d is not on the G%d curve" % (sid, name, index, 2 if g2 else 1), p, "compute")
    if sid != 6:
        last = (2 << p) - 1 if sid == 2 else (1 << p) - 1
        PKG.ptau_check(broken(**{"s%d" % sid: patched(body, unit * (last + 1), OFF_G2 if g2 else OFF_G1)}), p, "compute")


def test_prepared_points_are_checked_only_when_read():
    s = secs(True)
    n = 4  # p = 2: level 2 of sections 12 to 15 starts at point 3, M is level 3 of section 12 (from point 7), odd points
    for sid, unit, index in ((12, 64, 3), (12, 64, 6), (13, 128, 5), (14, 64, 4), (15, 64, 6), (12, 64, 8), (12, 64, 14)):
        bad = patched(s[sid], unit * index, OFF_G2 if unit == 128 else OFF_G1)
        data = broken(True, **{"s%d" % sid: bad})
        refuses(data, r"section %d \(lagrange \w+\) point %d is not on the G%d curve" % (sid, index, unit // 64), 2, "file")
        refuses(data, r"section %d .* point %d " % (sid, index), 2, "auto")
        PKG.ptau_check(data, 2, "compute")
    for index in (2, 7, 9, 13, 15):  # another level, and M's even points
        PKG.ptau_check(broken(True, s12=patched(s[12], 64 * index, OFF_G1)), 2, "file")
    assert n == 1 << 2
    # infinity is a point
    PKG.ptau_check(broken(True, s12=patched(s[12], 64 * 4, bytes(64))), 2, "file")


def test_domain_and_mode_refusals():
    plain, prep = PF.assemble(secs()), PF.assemble(secs(True))
    refuses(plain, r"domain 2\^3 needs a ceremony of power 4 or more, this file has power 3", 3)
    refuses(prep, r"needs a ceremony of power 5", 4, "file")
    refuses(plain, r"lagrange = file, but the file has no prepared sections", 2, "file")
    with pytest.raises(PKG.WitnessCalcError, match="lagrange must be one of"):
        PKG.ptau_check(plain, 2, "lazy")


# -- gwb_groth16_setup_ptau refuses before it touches the device ---------------------------------------------------------------
def _r1cs_bytes(n_constraints):
    rnd = random.Random(31)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(n_constraints)]
    pl = F.planted_system(rnd, 4, shapes, [1, R - 1, 2, None])
    return F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=0)


def test_setup_refuses_on_the_host():
    r2, r3 = PKG.R1cs(_r1cs_bytes(2)), PKG.R1cs(_r1cs_bytes(5))
    assert r2.qap_info()["domain_power"] == 2 and r3.qap_info()["domain_power"] == 3
    plain = PF.assemble(secs())
    s = secs()
    for args, pattern in (((r3, plain), r"needs a ceremony of power 4"), ((r2, plain, None, "file"), r"no prepared sections"),
                          ((r2, b"ptau"), r"bad magic"), ((r2, plain, 0), r"delta is not in \[1, r\)"), ((r2, plain, R), r"delta is not in"),
                          ((r2, broken(s6=patched(s[6], 0, OFF_G2))), r"section 6 \(betaG2\) point 0 is not on the G2 curve"),
                          ((r2, broken(s4=patched(s[4], 32, Q_BYTES))), r"section 4 \(alphaTauG1\) point 0 has a coordinate >= q"),
                          ((r2, broken(s3=s[3][:-128])), r"section 3 \(tauG2\) has 896 bytes, 1024 expected")):
        with pytest.raises(PKG.WitnessCalcError, match=pattern):
            PKG.groth16_setup_ptau(*args)
    with pytest.raises(PKG.WitnessCalcError, match="lagrange must be one of"):
        PKG.groth16_setup_ptau(r2, plain, 1, "lazy")
    with pytest.raises(PKG.WitnessCalcError, match="delta is not in"):
        PKG.groth16_setup_ptau(r2, plain, 1 << 256)


def _cli(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_cli_ptau_usage_and_file_errors(tmp_path):
    c, z, pt, t, d = (tmp_path / n for n in ("c.r1cs", "c.zkey", "pot.ptau", "t.txt", "d.txt"))
    c.write_bytes(_r1cs_bytes(2))
    pt.write_bytes(PF.assemble(secs()))
    t.write_text("5 7 11 13 17\n")
    d.write_text("12345\n")
    for args in (("--ptau", pt, "--trapdoor", t, c, z), ("--trapdoor", t, "--ptau", pt, c, z), ("--ptau", c, z), ("--ptau", pt, "--ptau", pt, c, z),
                 ("--delta", d, c, z), ("--delta", d, "--trapdoor", t, c, z), ("--ptau", pt, "--delta", c, z), ("--ptau", pt, "--lagrange", "lazy", c, z)):
        p = _cli(*args)
        assert p.returncode == 2 and "usage" in p.stderr, (args, p)
    p = _cli("--ptau", tmp_path / "missing.ptau", c, z)
    assert p.returncode == 2 and "cannot read" in p.stderr
    p = _cli("--ptau", c, c, z)
    assert p.returncode == 2 and "bad magic" in p.stderr
    (tmp_path / "c3.r1cs").write_bytes(_r1cs_bytes(5))
    p = _cli("--ptau", pt, tmp_path / "c3.r1cs", z)
    assert p.returncode == 2 and "needs a ceremony of power 4" in p.stderr
    p = _cli("--ptau", pt, "--lagrange", "file", c, z)
    assert p.returncode == 2 and "no prepared sections" in p.stderr
    for text, pattern in (("0\n", "delta is not in"), ("12 13\n", "1 expected"), ("0x12\n", "not a decimal integer"), ("", "1 expected")):
        d.write_text(text)
        p = _cli("--ptau", pt, "--delta", d, c, z)
        assert p.returncode == 2 and pattern in p.stderr, (text, p)
    assert not z.exists()
    assert struct.unpack_from("<I", pt.read_bytes(), 4)[0] == 1
