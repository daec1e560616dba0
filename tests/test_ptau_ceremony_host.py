"""The host side of the powers-of-tau ceremony (r1cs/ceremony.cc, include/graph_witness_groth16_ceremony.h) where there is no GPU:
ptau_new against the Python writer, section 7 written by tests/ceremony_fixtures.py and read by ptau_contributions with each of
the reader's refusals, the model of the device's signed-digit recoding, what ptau_contribute, ptau_verify and ptau_verify_step
refuse before they touch the device, and the powersoftau CLI's usage and file errors."""
import os
import random
import struct
import subprocess

import pytest

import cwc_import
from tests import ceremony_fixtures as CE
from tests import contribution_fixtures as CF
from tests import groth16_fixtures as GF
from tests import ptau_fixtures as PF

PKG = cwc_import.load()
R, Q = GF.R, GF.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "circom-witnesscalc_amd", "powersoftau")
TAU, ALPHA, BETA = (random.Random(900).randrange(2, R) for _ in range(3))


def refused(call, *args, **kw):
    with pytest.raises(PKG.WitnessCalcError) as e:
        call(*args, **kw)
    return str(e.value)


# -- ptau_new -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", [1, 3])
def test_a_new_file_is_the_file_of_the_logs_one(power):
    data = PKG.ptau_new(power)
    assert data == PF.write_ptau(power, 1, 1, 1)
    assert PKG.ptau_info(data) == {"power": power, "ceremony_power": power, "prepared": False, "n_contributions": 0}
    assert PKG.ptau_contributions(data) == []


@pytest.mark.parametrize("power", [0, 29])
def test_a_new_file_of_power_0_or_29_is_refused(power):
    assert "ptau new: power %d is not in [1, 28]" % power in refused(PKG.ptau_new, power)


# -- section 7 ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def records():
    """two records on top of a file of the logs (TAU, ALPHA, BETA), the second a beacon by its type and parameters"""
    secs = PF.sections(1, TAU, ALPHA, BETA)
    ch = CE.first_challenge(secs[1])
    a = CE.contribution(ch, (TAU, ALPHA, BETA), (3, 5, 7), (11, 13, 17), name="first")
    logs = (TAU * 3 % R, ALPHA * 5 % R, BETA * 7 % R)
    b = CE.contribution(a.next_challenge, logs, (19, 23, 29), (31, 37, 41))
    b.type, b.params = 1, CF.beacon_params("béacon", 10, bytes(range(32)))
    b.partial_hash = bytes(range(216))
    return [a, b]


def with_section7(body, power=1):
    secs = PF.sections(power, TAU, ALPHA, BETA)
    secs[7] = body
    return PF.assemble(secs)


def test_records_round_trip_through_the_reader(records):
    body = CE.write_section7(records)
    assert len(body) == 4 + 2 * CE.RECORD_FIXED + sum(len(r.params) for r in records)
    got = PKG.ptau_contributions(with_section7(body))
    assert len(got) == 2 and PKG.ptau_info(with_section7(body))["n_contributions"] == 2
    for rec, want in zip(got, records):
        for name, pt in want.canonical().items():
            assert rec[name] == pt, name
        assert rec["next_challenge"] == want.next_challenge and rec["type"] == want.type
    assert [r["name"] for r in got] == ["first", "béacon"]
    assert [CE.read_section7(body)[k].stored() for k in range(2)] == [r.stored() for r in records]
    # a file without section 7 has no records
    secs = PF.sections(1, TAU, ALPHA, BETA)
    del secs[7]
    assert PKG.ptau_contributions(PF.assemble(secs)) == []


def test_each_refusal_of_the_section_7_reader(records):
    a, b = records
    one, both = CE.write_section7([a]), CE.write_section7(records)
    p_a = len(a.params)

    def said(body):
        msg = refused(PKG.ptau_contributions, with_section7(body))
        assert msg.startswith("ptau: section 7"), msg
        return msg

    assert "is truncated (3 bytes, 4 at the least)" in said(b"\x01\x00\x00")
    assert "declares 2 contributions, which its %d bytes cannot hold" % len(one) in said(struct.pack("<I", 2) + one[4:])
    assert "declares 4294967295 contributions" in said(struct.pack("<I", 0xffffffff))
    # a count that fits by size while the first record's parameters push the second past the end
    padded = struct.pack("<I", 2) + one[4:] + bytes(CE.RECORD_FIXED - p_a)
    assert "contribution 2: the record is truncated" in said(padded)
    plen_at = 4 + CE.RECORD_FIXED - 4
    assert "contribution 1: paramsLen %d runs past the section's end (%d bytes left)" % (p_a + 1, p_a) in said(
        one[:plen_at] + struct.pack("<I", p_a + 1) + one[plen_at + 4:])
    assert "contribution 1: the length of parameter 01 runs past the parameters' end" in said(one[:plen_at + 5] + bytes([p_a]) + one[plen_at + 6:])
    assert "contribution 1: unknown parameter tag 9" in said(one[:plen_at + 4] + b"\x09" + one[plen_at + 5:])
    assert "contribution 2: paramsLen %d runs past the section's end (%d bytes left)" % (len(b.params), len(b.params) - 1) in said(both[:-1])
    short3 = CE.Record(b.pts, b.next_challenge, 1, bytes([3, 5, 1, 2]))  # 03 declares five bytes and has two
    assert "contribution 2: the length of parameter 03 runs past the parameters' end" in said(CE.write_section7([a, short3]))
    only2 = CE.Record(b.pts, b.next_challenge, 1, bytes([2]))  # 02 without its value
    assert "contribution 1: parameter 02 (numIterationsExp) runs past the parameters' end" in said(CE.write_section7([only2]))
    type_at = 4 + CE.RECORD_FIXED - 8
    assert "contribution 1: unknown type 2 (0 = contribution, 1 = beacon)" in said(one[:type_at] + struct.pack("<I", 2) + one[type_at + 4:])
    assert "has 1 trailing bytes after its last contribution" in said(one + b"\x00")
    # points: a coordinate >= q and a point off its curve, in an after-value, a G1 key point and a G2 key point
    offsets = {"tauG1": 4, "tauG2": 4 + 64, "beta_g1_sx": 4 + 448 + 5 * 64, "alpha_g2_spx": 4 + 448 + 384 + 128}
    for name, at in offsets.items():
        g2 = name.endswith("G2") or name.endswith("spx")
        big = one[:at] + Q.to_bytes(32, "little") + one[at + 32:]
        assert "contribution 1: %s has a coordinate >= q" % name in said(big)
        y_at = at + (64 if g2 else 32)
        off_curve = one[:y_at] + GF.lem(1) + one[y_at + 32:]
        assert "contribution 1: %s is not on the %s curve" % (name, "G2" if g2 else "G1") in said(off_curve)


# -- the recoding -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [3, 4, 5])
def test_the_signed_digits_of_the_edge_scalars(w):
    """sum d_j 2^(w j) = s, |d_j| <= 2^(w-1), the top digit holds what is left of s without a carry out of it, and the digits the
    kernel takes from s + C are those of the recoding from the bottom"""
    half, n = 1 << (w - 1), CE.windows(w)
    rnd = random.Random(910 + w)
    for s in CE.edge_scalars() + [rnd.randrange(R) for _ in range(300)]:
        d = CE.recode(s, w)
        assert len(d) == n and sum(x << (w * j) for j, x in enumerate(d)) == s
        assert all(-half <= x < half for x in d[:-1]) and 0 <= d[-1] <= half, hex(s)
        assert CE.recode_offset(s, w) == d, hex(s)


def test_the_top_digit_never_carries_out_for_any_scalar_below_r():
    """the top window of s < r is at most r's, and a carry into it comes from below it: the largest top digit over all s < r is
    reached at the largest s with that window, or at the largest s whose lower windows carry; both stay inside the table"""
    for w in (3, 4, 5):
        half, shift = 1 << (w - 1), w * (CE.windows(w) - 1)
        top = (R - 1) >> shift
        assert top + 1 <= half
        for s in (R - 1, (top << shift) - 1, ((top - 1) << shift) | ((1 << shift) - 1), (1 << shift) - 1):
            assert 0 <= CE.recode(s, w)[-1] <= half
    ripple = int("0" + "f" * 63, 16)  # the carry of the lowest window runs through every window up to the top one
    assert ripple < R and CE.recode(ripple, 4) == [-1] + [0] * 62 + [1]


# -- refusals made before the device is touched -------------------------------------------------------------------------------------
def test_contribute_and_verify_refuse_bad_input_before_the_device():
    good = PF.write_ptau(1, TAU, ALPHA, BETA)
    for call in (PKG.ptau_contribute, PKG.ptau_verify, PKG.ptau_contributions):
        assert "bad magic" in refused(call, b"zkey" + good[4:])
        assert refused(call, with_section7(b"\x01\x00\x00")).startswith("ptau: section 7 is truncated")
    assert "previous file: ptau: bad magic" in refused(PKG.ptau_verify_step, b"zkey" + good[4:], good)
    assert "next file: ptau: bad magic" in refused(PKG.ptau_verify_step, good, b"zkey" + good[4:])
    for j, nm in enumerate(("tau", "alpha", "beta")):
        for bad in (0, R, (1 << 256) - 1):
            secrets = [2, 3, 5]
            secrets[j] = bad
            assert "the secret %s is not in [1, r)" % nm in refused(PKG.ptau_contribute, good, secrets=secrets)
    assert "secrets: three integers" in refused(PKG.ptau_contribute, good, secrets=(1, 2))
    assert "the name has 256 bytes, 255 at the most" in refused(PKG.ptau_contribute, good, name="n" * 256, secrets=(2, 3, 5))
    assert "seed: 32 bytes expected" in refused(PKG.ptau_verify, good, seed=b"short")
    secs = PF.sections(1, TAU, ALPHA, BETA)
    secs[6] = GF.lem(1) + secs[6][32:]
    assert "ptau: section 6 (betaG2) point 0 is not on the G2 curve" in refused(PKG.ptau_contribute, PF.assemble(secs), secrets=(2, 3, 5))
    assert "ptau: section 6 (betaG2) point 0 is not on the G2 curve" in refused(PKG.ptau_verify, PF.assemble(secs))
    secs = PF.sections(1, TAU, ALPHA, BETA)
    secs[4] = secs[4][:64] + Q.to_bytes(32, "little") + secs[4][96:]
    assert "ptau: section 4 (alphaTauG1) point 1 has a coordinate >= q" in refused(PKG.ptau_verify, PF.assemble(secs))
    assert "next file: ptau: section 4 (alphaTauG1) point 1 has a coordinate >= q" in refused(PKG.ptau_verify_step, good, PF.assemble(secs))


# -- the CLI ------------------------------------------------------------------------------------------------------------------------
def run(*args):
    p = subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout, p.stderr


def test_cli_usage_and_file_errors_exit_2(tmp_path):
    path = lambda n: str(tmp_path / n)  # noqa: E731
    for args in ([], ["new"], ["new", "3"], ["new", "x", path("a.ptau")], ["contribute", path("a.ptau")], ["verify"], ["verify", "--name", "n", path("a.ptau")],
                 ["verify-step", path("a.ptau")], ["beacon", path("a.ptau"), path("b.ptau")], ["contribute", "--frobnicate", path("a.ptau"), path("b.ptau")],
                 ["new", "--skip-records", "3", path("a.ptau")]):
        rc, _, err = run(*args)
        assert rc == 2 and "usage: powersoftau new POWER <out.ptau>" in err and "powersoftau verify-step <prev.ptau> <next.ptau>" in err, args
    rc, _, err = run("new", "0", path("a.ptau"))
    assert rc == 2 and "ptau new: power 0 is not in [1, 28]" in err
    rc, _, err = run("new", "2", path("no/such/dir/a.ptau"))
    assert rc == 2 and "cannot write" in err
    rc, out, _ = run("new", "2", path("a.ptau"))
    assert rc == 0 and out == "" and open(path("a.ptau"), "rb").read() == PF.write_ptau(2, 1, 1, 1)
    for args in (["contribute", path("missing.ptau"), path("b.ptau")], ["verify", path("missing.ptau")], ["verify-step", path("a.ptau"), path("missing.ptau")],
                 ["verify-step", path("missing.ptau"), path("a.ptau")]):
        rc, _, err = run(*args)
        assert rc == 2 and "cannot read" in err and "missing.ptau" in err, args
    open(path("junk.ptau"), "wb").write(b"not a ptau file at all")
    for args in (["contribute", path("junk.ptau"), path("b.ptau")], ["verify", path("junk.ptau")], ["verify-step", path("a.ptau"), path("junk.ptau")]):
        rc, _, err = run(*args)
        assert rc == 2 and "error: " in err and "ptau: bad magic" in err, args
    open(path("s.txt"), "w").write("2 3\n")
    rc, _, err = run("contribute", "--secrets", path("s.txt"), path("a.ptau"), path("b.ptau"))
    assert rc == 2 and "three decimal integers below 2^256 expected" in err
    open(path("s.txt"), "w").write("2 0 3\n")
    rc, _, err = run("contribute", "--secrets", path("s.txt"), path("a.ptau"), path("b.ptau"))
    assert rc == 2 and "the secret alpha is not in [1, r)" in err
    assert not os.path.exists(path("b.ptau"))


# -- the section 7 reader under ASan and UBSan ----------------------------------------------------------------------------------------
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FLIPS = 300


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/native/ceremony_host.cc over ceremony.cc, ptau.cc and contributions.cc: a stand-alone CPU program, no device"""
    exe = str(tmp_path_factory.mktemp("ceremony_host") / "ceremony_host")
    src = os.path.join(ROOT, "circom-witnesscalc_amd", "r1cs")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(ROCM, "include"), "-o", exe, os.path.join(ROOT, "tests", "native", "ceremony_host.cc")]
                          + [os.path.join(src, f) for f in ("ceremony.cc", "ptau.cc", "contributions.cc")])
    return exe


def xorshift64(x):
    while True:
        x ^= (x << 13) & 0xffffffffffffffff
        x ^= x >> 7
        x ^= (x << 17) & 0xffffffffffffffff
        yield x


def test_the_reader_on_truncations_and_on_flipped_bytes_under_sanitizers(host_program, records, tmp_path):
    """the honest section, every third of its prefixes and 300 one-byte changes: the sanitized build reads nothing outside the file,
    and says for every case what the library says"""
    body = CE.write_section7(records)
    (tmp_path / "base.ptau").write_bytes(with_section7(body))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([host_program, str(tmp_path / "base.ptau"), str(FLIPS)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.split("\n")[:-1]
    rnd = xorshift64(88172645463325252)
    cases = [body] + [body[:cut] for cut in range(0, len(body), 3)]
    for _ in range(FLIPS):
        at, value = next(rnd) % len(body), next(rnd) & 0xff
        cases.append(body[:at] + bytes([value]) + body[at + 1:])
    assert len(lines) == len(cases)
    accepted = 0
    for case, line in zip(cases, lines):
        try:
            PKG.ptau_contributions(with_section7(case))
            accepted += 1
            assert line.startswith("0 "), line
        except PKG.WitnessCalcError as e:
            assert line == "2 " + str(e) and str(e).startswith("ptau: section 7"), (line, str(e))
    assert 1 <= accepted <= 1 + FLIPS  # the honest section, and flips that leave a hash or a name another value
