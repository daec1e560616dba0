"""The host side of the random beacon (r1cs/beacon.hpp, include/graph_witness_groth16_beacon.h) where there is no GPU: SHA-256
against hashlib at the padding edges, the derived scalars against tests/beacon_fixtures.py, every refusal that the making and the
verifying calls make before they touch the device (here they arrive as their messages, not as a device error), the beacon's
parameters in the record lists, the CLIs' usage and hex errors, and beacon.hpp under ASan and UBSan."""
import ctypes
import functools
import hashlib
import os
import random
import struct
import subprocess
import sys

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
TAU, ALPHA, BETA = (random.Random(1200).randrange(2, R) for _ in range(3))
HASH = bytes(range(1, 33))
CON = ([(1, 1)], [(2, 1)], [(3, 1)])  # w1 w2 = w3


def refused(call, *args, **kw):
    with pytest.raises(PKG.WitnessCalcError) as e:
        call(*args, **kw)
    return str(e.value)


# -- SHA-256 and the derivation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 1, 55, 56, 63, 64, 65, 119, 120, 1000))
def test_sha256_at_the_padding_edges(n):
    data = bytes(random.Random(n).randrange(256) for _ in range(n))
    assert PKG.sha256(data) == hashlib.sha256(data).digest()


@pytest.mark.parametrize("hash_len", (1, 32, 255))
@pytest.mark.parametrize("exp", (10, 12))
@pytest.mark.parametrize("phase", (1, 2))
def test_beacon_scalars_are_the_fixtures(phase, exp, hash_len):
    digest = bytes(random.Random(hash_len).randrange(256) for _ in range(hash_len))
    got = PKG.beacon_scalars(phase, digest, exp)
    assert got == BF.scalars(phase, digest, exp) and len(got) == (6 if phase == 1 else 2)
    assert all(1 <= x < R for x in got) and len(set(got)) == len(got)


def test_beacon_scalars_refuse_what_the_making_calls_refuse():
    for args in ((0, HASH, 10), (3, HASH, 10), (1, b"", 10), (1, bytes(256), 10), (1, HASH, 9), (2, HASH, 64), (2, HASH, 29)):
        assert refused(PKG.beacon_scalars, *args).startswith("beacon: phase 1 or 2"), args


# -- files ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def good_ptau():
    return PF.write_ptau(1, TAU, ALPHA, BETA)


def ptau_with(records, power=1):
    secs = PF.sections(power, TAU, ALPHA, BETA)
    secs[7] = CE.write_section7(records)
    return PF.assemble(secs)


@functools.lru_cache(maxsize=None)
def ptau_record():
    secs = PF.sections(1, TAU, ALPHA, BETA)
    return CE.contribution(CE.first_challenge(secs[1]), (1, 1, 1), (TAU, ALPHA, BETA), (11, 13, 17), name="first")


def ptau_beacon_with(params):
    r = ptau_record()
    return ptau_with([CE.Record(r.pts, r.next_challenge, 1, params)])


def with_section10(zkey, body):
    n_sec = struct.unpack_from("<I", zkey, 8)[0]
    off, out = 12, b""
    for _ in range(n_sec):
        sid, size = struct.unpack_from("<IQ", zkey, off)
        out += GF.section(sid, body if sid == 10 else zkey[off + 12:off + 12 + size])
        off += 12 + size
    return zkey[:12] + out


@functools.lru_cache(maxsize=None)
def blank_key():
    return with_section10(GF.Trapdoor([CON], 4, 0, seed=5).zkey, CF.NO_RECORDS)


@functools.lru_cache(maxsize=None)
def zkey_record():
    return CF.contribution(bytes(range(64)), [], GF.G1_GEN, 12345, 678, name="first")


def zkey_beacon_with(params):
    r = zkey_record()
    rec = CF.Record(r.delta_after, r.g1_s, r.g1_sx, r.g2_spx, r.transcript, 1, params)
    return with_section10(blank_key(), CF.write_section10(bytes(range(64)), [rec]))


# -- the making calls' refusals ----------------------------------------------------------------------------------------------------
def test_each_refusal_of_the_making_calls_comes_before_the_device():
    for call, image in ((PKG.ptau_beacon, good_ptau()), (PKG.groth16_beacon, blank_key())):
        assert refused(call, image, HASH, 9) == "beacon: numIterationsExp 9 is not in [10, 63]"
        assert refused(call, image, HASH, 64) == "beacon: numIterationsExp 64 is not in [10, 63]"
        assert refused(call, image, HASH, 29) == "beacon: numIterationsExp 29 is above the limit 28 (CWC_BEACON_MAX_EXP)"
        assert refused(call, image, b"", 10) == "beacon: the beaconHash is empty"
        assert refused(call, image, bytes(256), 10) == "beacon: the beaconHash has 256 bytes, 255 at the most"
        assert refused(call, image, HASH, 10, name="n" * 256) == "beacon: the name has 256 bytes, 255 at the most"
        assert "the name holds a zero byte" in refused(call, image, HASH, 10, name="a\0b")
    # what contribute refuses about the file, with its messages
    assert "bad magic" in refused(PKG.ptau_beacon, b"zkey" + good_ptau()[4:], HASH, 10)
    secs = PF.sections(1, TAU, ALPHA, BETA)
    secs[7] = b"\x01\x00\x00"
    assert refused(PKG.ptau_beacon, PF.assemble(secs), HASH, 10).startswith("ptau: section 7 is truncated")
    secs = PF.sections(1, TAU, ALPHA, BETA)
    secs[6] = GF.lem(1) + secs[6][32:]
    assert "ptau: section 6 (betaG2) point 0 is not on the G2 curve" in refused(PKG.ptau_beacon, PF.assemble(secs), HASH, 10)
    assert refused(PKG.groth16_beacon, b"not a key at all", HASH, 10).startswith("zkey")
    assert refused(PKG.groth16_beacon, GF.Trapdoor([CON], 4, 0, seed=5).zkey, HASH, 10).startswith("zkey: section 10")  # an empty section 10
    # through the C ABI every one of them returns 2
    L, st = PKG.r1cs_lib(), PKG.GwStatus()
    out, n, digest = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.create_string_buffer(64)
    for call, image in ((L.gwb_ptau_beacon, good_ptau()), (L.gwb_groth16_beacon, blank_key())):
        assert call(image, len(image), b"", HASH, len(HASH), 64, ctypes.byref(out), ctypes.byref(n), digest, ctypes.byref(st)) == 2
        assert call(image, len(image), b"", None, 3, 10, ctypes.byref(out), ctypes.byref(n), digest, ctypes.byref(st)) == 2
        assert ctypes.string_at(st.error_msg).endswith(b"_beacon: NULL argument")


_LIMIT_SCRIPT = """
import sys
sys.path.insert(0, %r)
import cwc_import
PKG = cwc_import.load()
from tests import test_beacon_host as T
for call, image in ((PKG.ptau_beacon, T.good_ptau()), (PKG.groth16_beacon, T.blank_key())):
    print(T.refused(call, image, T.HASH, 11))
print(T.refused(PKG.ptau_verify, T.ptau_beacon_with(T.CF.beacon_params("", 11, T.HASH))))
print(T.refused(PKG.groth16_verify_contributions, T.zkey_beacon_with(T.CF.beacon_params("", 11, T.HASH))))
"""


def test_the_limit_is_the_environments(tmp_path):
    """CWC_BEACON_MAX_EXP = 10 in a child process (the knob is read once): e = 11 is refused by the making and the verifying calls"""
    (tmp_path / "limit.py").write_text(_LIMIT_SCRIPT % ROOT)
    env = dict(os.environ, CWC_BEACON_MAX_EXP="10")
    p = subprocess.run([sys.executable, str(tmp_path / "limit.py")], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p
    said = "numIterationsExp 11 is above the limit 10 (CWC_BEACON_MAX_EXP)"
    assert p.stdout.splitlines() == ["beacon: " + said] * 2 + ["ptau: contribution 1: " + said, "zkey: contribution 1: " + said]


# -- the verifying calls' refusals -------------------------------------------------------------------------------------------------
NEEDS = "a beacon record needs numIterationsExp and beaconHash"
FORMS = ((CF.name_params("b") + bytes([3, 2, 7, 7]), 1, NEEDS),                                      # no item 02
         (bytes([2, 10]), 1, NEEDS),                                                                  # no item 03
         (b"", 1, NEEDS),
         (bytes([2, 10, 3, 0]), 1, "a beacon record's beaconHash is empty"),
         (bytes([2, 10, 2, 10, 3, 1, 7]), 1, "a beacon record has more than one numIterationsExp or beaconHash"),
         (CF.beacon_params("", 9, HASH), 1, "numIterationsExp 9 is not in [10, 63]"),
         (CF.beacon_params("", 64, HASH), 1, "numIterationsExp 64 is not in [10, 63]"),
         (CF.beacon_params("b", 40, HASH), 2, "numIterationsExp 40 is above the limit 28 (CWC_BEACON_MAX_EXP)"))


def verdict(call, *args):
    st = PKG.GwStatus()
    rc = call(*args, ctypes.byref(st))
    return rc, ctypes.string_at(st.error_msg).decode() if st.error_msg else ""


@pytest.mark.parametrize("params,rc,msg", FORMS)
def test_the_verifications_refuse_a_malformed_beacon_record_before_the_device(params, rc, msg):
    L = PKG.r1cs_lib()
    image, prev = ptau_beacon_with(params), good_ptau()
    n = ctypes.c_size_t(0)
    assert verdict(L.gwb_ptau_verify, image, len(image), 0, None, None, ctypes.byref(n)) == (rc, "ptau: contribution 1: " + msg)
    assert verdict(L.gwb_ptau_verify_step, prev, len(prev), image, len(image), None) == (rc, "ptau: contribution 1: " + msg)
    key, prev = zkey_beacon_with(params), blank_key()
    assert verdict(L.gwb_zkey_verify_contributions, key, len(key), None, ctypes.byref(n)) == (rc, "zkey: contribution 1: " + msg)
    r1, pt = PKG.R1cs(F.write_r1cs(4, [CON])), PF.write_ptau(2, 5, 7, 11)
    want = ("zkey verify: " if rc == 1 else "zkey: ") + "contribution 1: " + msg
    assert verdict(L.gwb_zkey_verify_key, key, len(key), r1._h, pt, len(pt), 2, 0, None, None, ctypes.byref(n)) == (rc, want)
    # a verification that passes over the records passes over this rule: what comes next here is the device
    rc2, msg2 = verdict(L.gwb_ptau_verify, image, len(image), PKG.PTAU_VERIFY_SKIP_RECORDS, None, None, ctypes.byref(n))
    assert "contribution 1" not in msg2


def test_a_step_refuses_a_malformed_new_beacon_record():
    """the step's structure rules come first; they hold for a key whose csHash the previous blank key gives"""
    prev = blank_key()
    secs = {}
    n_sec, off = struct.unpack_from("<I", prev, 8)[0], 12
    for _ in range(n_sec):
        sid, size = struct.unpack_from("<IQ", prev, off)
        secs[sid] = prev[off + 12:off + 12 + size]
        off += 12 + size
    cs_hash = CF.H(b"".join(secs[i] for i in range(1, 10)))
    r = zkey_record()
    rec = CF.Record(r.delta_after, r.g1_s, r.g1_sx, r.g2_spx, r.transcript, 1, bytes([2, 10]))
    nxt = with_section10(prev, CF.write_section10(cs_hash, [rec]))
    assert verdict(PKG.r1cs_lib().gwb_zkey_verify_step, prev, len(prev), nxt, len(nxt), None) == (1, "zkey: contribution 1: " + NEEDS)


# -- the record lists ---------------------------------------------------------------------------------------------------------------
def test_the_record_lists_expose_a_beacons_parameters():
    a = ptau_record()
    b = CE.Record(a.pts, a.next_challenge, 1, CF.beacon_params("béacon", 10, bytes(range(32))))
    c = CE.Record(a.pts, a.next_challenge, 1, bytes([3, 1, 9]))  # a beacon by its type, without item 02
    got = PKG.ptau_contributions(ptau_with([a, b, c]))
    assert [(r["type"], r["iterations_exp"], r["beacon_hash"]) for r in got] == [(0, None, None), (1, 10, bytes(range(32))), (1, None, b"\x09")]
    assert [r["name"] for r in got] == ["first", "béacon", ""]
    z = zkey_record()
    recs = [z, CF.Record(z.delta_after, z.g1_s, z.g1_sx, z.g2_spx, z.transcript, 1, CF.beacon_params("beacon", 63, b"\xff" * 255))]
    got = PKG.zkey_contributions(with_section10(blank_key(), CF.write_section10(bytes(64), recs)))["contributions"]
    assert [(r["type"], r["iterations_exp"], r["beacon_hash"]) for r in got] == [(0, None, None), (1, 63, b"\xff" * 255)]
    assert [r["name"] for r in got] == ["first", "beacon"]
    # the raw parameters, and a record that is not there
    L, image = PKG.r1cs_lib(), ptau_with([a, b])
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    assert verdict(L.gwb_ptau_contribution_params, image, len(image), 1, ctypes.byref(out), ctypes.byref(n)) == (0, "")
    assert ctypes.string_at(out, n.value) == b.params
    L.gwb_groth16_setup_free(out)
    assert verdict(L.gwb_ptau_contribution_params, image, len(image), 2, ctypes.byref(out), ctypes.byref(n)) == (
        2, "ptau: there is no contribution 3 (the file has 2)")
    key = blank_key()
    assert verdict(L.gwb_zkey_contribution_params, key, len(key), 0, ctypes.byref(out), ctypes.byref(n)) == (
        2, "zkey: there is no contribution 1 (the key has 0)")


# -- the CLIs -----------------------------------------------------------------------------------------------------------------------
def run(tool, *args):
    p = subprocess.run([os.path.join(BIN, tool)] + list(args), capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout, p.stderr


def test_cli_usage_and_hex_errors_exit_2(tmp_path):
    path = lambda n: str(tmp_path / n)  # noqa: E731
    (tmp_path / "a.ptau").write_bytes(good_ptau())
    (tmp_path / "k.zkey").write_bytes(blank_key())
    for args in (["beacon"], ["beacon", path("a.ptau"), path("b.ptau"), "00"], ["beacon", path("a.ptau"), path("b.ptau"), "00", "10", "x"],
                 ["beacon", "--secrets", path("s"), path("a.ptau"), path("b.ptau"), "00", "10"], ["contribute", "--require-beacon", path("a.ptau"), path("b.ptau")],
                 ["verify", "--require-beacon"]):
        rc, _, err = run("powersoftau", *args)
        assert rc == 2 and "usage: powersoftau new POWER <out.ptau>" in err and "powersoftau verify-step <prev.ptau> <next.ptau>" in err, args
        assert "powersoftau beacon [--name NAME] <in.ptau> <out.ptau> <beaconHash(hex)> <numIterationsExp>" in err
        assert "powersoftau verify [--skip-records] <file.ptau>" in err and "--require-beacon <file.ptau>" in err
    for args in (["--beacon", path("k.zkey"), path("o.zkey"), "00"], ["--beacon", "--delta", path("d"), path("k.zkey"), path("o.zkey"), "00", "10"],
                 ["--beacon", "--verify", path("k.zkey")], ["--require-beacon", path("k.zkey"), path("o.zkey")], ["--verify-step", "--require-beacon", path("k.zkey"), path("o.zkey")]):
        rc, _, err = run("groth16-contribute", *args)
        assert rc == 2 and "usage: groth16-contribute [--name NAME] [--delta FILE] <in.zkey> <out.zkey>" in err, args
        assert "groth16-contribute --beacon [--name NAME] <in.zkey> <out.zkey> <beaconHash(hex)> <numIterationsExp>" in err
        assert "groth16-contribute --verify <key.zkey>" in err and "groth16-contribute --verify-step <prev.zkey> <next.zkey>" in err
    for bad in ("", "0", "abc", "0x00", "zz", "00 ", "ab" * 256):
        rc, _, err = run("powersoftau", "beacon", path("a.ptau"), path("b.ptau"), bad, "10")
        assert rc == 2 and err.startswith("error: beaconHash: "), bad
        rc, _, err = run("groth16-contribute", "--beacon", path("k.zkey"), path("o.zkey"), bad, "10")
        assert rc == 2 and err.startswith("error: beaconHash: "), bad
    for bad in ("", "ten", "10x"):
        rc, _, err = run("powersoftau", "beacon", path("a.ptau"), path("b.ptau"), "00", bad)
        assert rc == 2 and err.startswith("error: numIterationsExp: "), bad
        rc, _, err = run("groth16-contribute", "--beacon", path("k.zkey"), path("o.zkey"), "00", bad)
        assert rc == 2 and err.startswith("error: numIterationsExp: "), bad
    # a good hex argument in either case reaches the library, whose refusal of the exponent exits 2 as well
    rc, _, err = run("powersoftau", "beacon", path("a.ptau"), path("b.ptau"), "aBcD", "9")
    assert rc == 2 and err == "error: beacon: numIterationsExp 9 is not in [10, 63]\n"
    rc, _, err = run("groth16-contribute", "--beacon", path("k.zkey"), path("o.zkey"), "ab" * 255, "64")
    assert rc == 2 and err == "error: beacon: numIterationsExp 64 is not in [10, 63]\n"
    rc, _, err = run("powersoftau", "beacon", path("missing.ptau"), path("b.ptau"), "00", "10")
    assert rc == 2 and "cannot read" in err
    assert not os.path.exists(path("b.ptau")) and not os.path.exists(path("o.zkey"))
    # groth16-setup --export-vk
    for args in (["--export-vk"], ["--export-vk", path("k.zkey")], ["--export-vk", path("k.zkey"), path("vk.json"), "x"], ["--export-vk", "--ptau", path("vk.json")]):
        rc, _, err = run("groth16-setup", *args)
        assert rc == 2 and "--export-vk <key.zkey> <verification_key.json>" in err and "--prepare-ptau <in.ptau> <out.ptau>" in err, args
    rc, _, err = run("groth16-setup", "--export-vk", path("missing.zkey"), path("vk.json"))
    assert rc == 2 and "cannot read" in err
    (tmp_path / "junk.zkey").write_bytes(b"not a key at all")
    rc, _, err = run("groth16-setup", "--export-vk", path("junk.zkey"), path("vk.json"))
    assert rc == 2 and "error: " in err and "zkey" in err and not os.path.exists(path("vk.json"))


# -- beacon.hpp under ASan and UBSan ------------------------------------------------------------------------------------------------
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FLIPS = 300


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/native/beacon_host.cc over ceremony.cc, ptau.cc and contributions.cc: a stand-alone CPU program, no device"""
    exe = str(tmp_path_factory.mktemp("beacon_host") / "beacon_host")
    src = os.path.join(ROOT, "circom-witnesscalc_amd", "r1cs")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(ROCM, "include"), "-o", exe, os.path.join(ROOT, "tests", "native", "beacon_host.cc")]
                          + [os.path.join(src, f) for f in ("ceremony.cc", "ptau.cc", "contributions.cc")])
    return exe


def xorshift64(x):
    while True:
        x ^= (x << 13) & 0xffffffffffffffff
        x ^= x >> 7
        x ^= (x << 17) & 0xffffffffffffffff
        yield x


def model(par, limit=28):
    """the line beacon_host prints for the parameter bytes `par`: read_params and form_of, restated"""
    ok, n_exp, n_hash, exp, hash_len, i = 1, 0, 0, 0, 0, 0
    while i < len(par):
        tag = par[i]
        i += 1
        if tag == 2:
            if i >= len(par):
                ok = 0
                break
            exp, n_exp, i = par[i], n_exp + 1, i + 1
        elif tag in (1, 3):
            if i >= len(par) or par[i] > len(par) - i - 1:
                ok = 0
                break
            if tag == 3:
                hash_len, n_hash = par[i], n_hash + 1
            i += 1 + par[i]
        else:
            ok = 0
            break
    if not ok or n_exp != 1 or n_hash != 1 or hash_len == 0 or not 10 <= exp <= 63:
        rc = 1
    else:
        rc = 2 if exp > limit else 0
    return "%d %d %d %d %d %d" % (ok, n_exp, n_hash, exp, hash_len, rc)


def test_beacon_hpp_under_sanitizers(host_program):
    """SHA-256's vectors, the chain's one-block links, the derivation against the fixture, and the parameter reader on the honest
    parameters, every prefix of them and 300 one-byte changes: the sanitized build reads nothing outside them"""
    digest, exp, name = bytes(range(200, 232)), 11, "béacon"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([host_program, digest.hex(), str(exp), name, str(FLIPS)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.split("\n")[:-1]
    assert lines[0] == "chain " + BF.chain(digest, exp).hex()
    for phase in (1, 2):
        assert lines[phase] == "scalars%d " % phase + " ".join(x.to_bytes(32, "little").hex() for x in BF.scalars(phase, digest, exp))
    body = CF.beacon_params(name, exp, digest)
    assert lines[3] == "params " + body.hex()
    cases = [body] + [body[:cut] for cut in range(len(body))]
    rnd = xorshift64(88172645463325252)
    for _ in range(FLIPS):
        at, value = next(rnd) % len(body), next(rnd) & 0xff
        cases.append(body[:at] + bytes([value]) + body[at + 1:])
    assert len(lines) == 4 + len(cases)
    assert [model(c) for c in cases] == lines[4:]
    # the honest parameters pass, no proper prefix of them does, and some of the changed ones (a byte of the hash or the name) do
    assert lines[4].endswith(" 0") and all(ln.endswith(" 1") for ln in lines[5:5 + len(body)])
    assert 0 < sum(ln.endswith(" 0") for ln in lines[5 + len(body):]) < FLIPS
