"""The parts of the key check (gwb_zkey_verify_key, include/graph_witness_groth16_contribute.h) and of the powers check
(gwb_ptau_check_powers, include/graph_witness_groth16_ptau.h) that run before the device is touched: NULL arguments, bytes that
are no key or no `.ptau`, a circuit too large for the file, the size rule, the Python arguments and the CLI's usage errors.  Keys
come from groth16_fixtures.Trapdoor and the `.ptau` from ptau_fixtures, both on the plain-Python curve; none of them is an
honest key of the file, which no rule that runs here looks at."""
import ctypes
import functools
import os
import struct
import subprocess

import pytest

import cwc_import
from tests import contribution_fixtures as CF
from tests import groth16_fixtures as GF
from tests import ptau_fixtures as PF
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "circom-witnesscalc_amd", "groth16-contribute")
CON = ([(1, 1)], [(2, 1)], [(3, 1)])  # w1 w2 = w3


@functools.lru_cache(maxsize=None)
def ptau():
    return PF.write_ptau(2, 5, 7, 11)


def with_section10(zkey, body):
    """the key with its section 10 replaced (the fixture writes an empty one, which the reader of the records refuses)"""
    n_sec = struct.unpack_from("<I", zkey, 8)[0]
    off, out = 12, b""
    for _ in range(n_sec):
        sid, size = struct.unpack_from("<IQ", zkey, off)
        out += GF.section(sid, body if sid == 10 else zkey[off + 12:off + 12 + size])
        off += 12 + size
    return zkey[:12] + out


@functools.lru_cache(maxsize=None)
def key(n_constraints=1, n_wires=4, n_pub=0):
    return with_section10(GF.Trapdoor([CON] * n_constraints, n_wires, n_pub, seed=5).zkey, CF.NO_RECORDS)


def circuit(n_constraints=1, n_wires=4):
    return PKG.R1cs(F.write_r1cs(n_wires, [CON] * n_constraints))


def call(zkey, r1, pt, mode=2, flags=0, n=0, hashes=None, n_null=False):
    st = PKG.GwStatus()
    count = ctypes.c_size_t(n)
    rc = PKG.r1cs_lib().gwb_zkey_verify_key(zkey, len(zkey) if zkey is not None else 5, r1._h if r1 is not None else None, pt,
                                            len(pt) if pt is not None else 5, mode, flags, None, hashes, None if n_null else ctypes.byref(count),
                                            ctypes.byref(st))
    msg = ctypes.string_at(st.error_msg).decode() if st.error_msg else ""
    return rc, msg


def test_null_arguments():
    r1 = circuit()
    for args in ((None, r1, ptau()), (key(), None, ptau()), (key(), r1, None)):
        assert call(*args) == (2, "gwb_zkey_verify_key: NULL argument")
    assert call(key(), r1, ptau(), n_null=True) == (2, "gwb_zkey_verify_key: NULL argument")
    assert call(key(), r1, ptau(), n=1, hashes=None) == (2, "gwb_zkey_verify_key: NULL argument")
    assert call(key(), r1, ptau(), flags=4) == (2, "gwb_zkey_verify_key: unknown flags 4")
    st = PKG.GwStatus()
    assert PKG.r1cs_lib().gwb_ptau_check_powers(None, 5, 1, None, ctypes.byref(st)) == 2
    assert ctypes.string_at(st.error_msg) == b"gwb_ptau_check_powers: NULL argument"
    st = PKG.GwStatus()
    assert PKG.r1cs_lib().gwb_bn254_g2_lincomb128_device(None, None, 0, None, None, ctypes.byref(st)) == 1
    assert ctypes.string_at(st.error_msg) == b"gwb_bn254_g2_lincomb128_device: NULL argument"


def test_bytes_that_are_no_key_or_no_ptau():
    r1 = circuit()
    rc, msg = call(b"not a key at all", r1, ptau())
    assert rc == 2 and msg.startswith("zkey")
    rc, msg = call(GF.Trapdoor([CON], 4, 0, seed=5).zkey, r1, ptau())  # an empty section 10
    assert rc == 2 and msg.startswith("zkey: section 10")
    rc, msg = call(key(), r1, b"ptau" + bytes(20))
    assert rc == 2 and msg.startswith("ptau")
    rc, msg = call(key(), r1, ptau()[:-1])
    assert rc == 2 and msg.startswith("ptau")
    rc, msg = call(key(), r1, ptau(), mode=3)
    assert rc == 2 and msg.startswith("ptau: lagrange mode 3")
    rc, msg = call(key(), r1, ptau(), mode=1)
    assert rc == 2 and msg.startswith("ptau: lagrange = file, but the file has no prepared sections")
    st = PKG.GwStatus()
    assert PKG.r1cs_lib().gwb_ptau_check_powers(b"ptau" + bytes(20), 24, 1, None, ctypes.byref(st)) == 2
    assert ctypes.string_at(st.error_msg).startswith(b"ptau")
    with pytest.raises(PKG.WitnessCalcError, match="^ptau"):
        PKG.ptau_check_powers(ptau()[:-1], 1)
    with pytest.raises(PKG.WitnessCalcError, match="^ptau: the circuit's domain 2\\^2 needs a ceremony of power 3 or more"):
        PKG.ptau_check_powers(ptau(), 2)


def test_circuit_too_large_for_the_file():
    """three constraints: domain 2^2, for which a file of power 2 is one power short; the setup's message, before the sizes"""
    rc, msg = call(key(), circuit(n_constraints=3), ptau())
    assert rc == 2 and msg.startswith("ptau: the circuit's domain 2^2 needs a ceremony of power 3 or more, this file has power 2")
    with pytest.raises(PKG.WitnessCalcError, match="^ptau: the circuit's domain 2\\^2 needs"):
        PKG.groth16_verify_key(key(), circuit(n_constraints=3), ptau())


def test_size_mismatches():
    r1 = circuit()
    assert call(key(n_wires=5), r1, ptau()) == (1, "zkey verify: nVars of the key is 5, the circuit's is 4")
    assert call(key(n_pub=1), r1, ptau()) == (1, "zkey verify: nPublic of the key is 1, the circuit's is 0")
    assert call(key(n_constraints=2), r1, ptau()) == (1, "zkey verify: domainSize of the key is 4, the circuit's is 2")
    with pytest.raises(PKG.WitnessCalcError, match="^zkey verify: nVars of the key is 5, the circuit's is 4$"):
        PKG.groth16_verify_key(key(n_wires=5), r1, ptau(), records=False, check_ptau=True)


def test_python_arguments():
    r1 = circuit()
    with pytest.raises(PKG.WitnessCalcError, match="^lagrange must be one of"):
        PKG.groth16_verify_key(key(), r1, ptau(), lagrange="bogus")
    for seed in (b"", bytes(31), bytes(33)):
        with pytest.raises(PKG.WitnessCalcError, match="^seed: 32 bytes expected$"):
            PKG.groth16_verify_key(key(), r1, ptau(), seed=seed)
        with pytest.raises(PKG.WitnessCalcError, match="^seed: 32 bytes expected$"):
            PKG.ptau_check_powers(ptau(), 1, seed=seed)
    with pytest.raises(PKG.WitnessCalcError, match="^zkey"):
        PKG.groth16_verify_key(b"zkey", r1, ptau())
    # a bytearray and a memoryview are buffers too
    with pytest.raises(PKG.WitnessCalcError, match="^zkey verify: nVars"):
        PKG.groth16_verify_key(key(n_wires=5), r1, bytearray(ptau()))
    with pytest.raises(PKG.WitnessCalcError, match="^zkey verify: nVars"):
        PKG.groth16_verify_key(key(n_wires=5), r1, memoryview(ptau()))


def _cli(*args):
    p = subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=60)
    return p.returncode, p.stderr


def test_cli_usage_and_files(tmp_path):
    (tmp_path / "c.r1cs").write_bytes(F.write_r1cs(4, [CON]))
    (tmp_path / "pot.ptau").write_bytes(ptau())
    (tmp_path / "k.zkey").write_bytes(key(n_wires=5))
    (tmp_path / "junk.zkey").write_bytes(b"junk")
    c, p, k, junk = (str(tmp_path / n) for n in ("c.r1cs", "pot.ptau", "k.zkey", "junk.zkey"))
    for args in (("--verify-key", c, p), ("--verify-key", c, p, k, k), ("--verify-key", "--lagrange", "bogus", c, p, k),
                 ("--verify-key", "--verify", c, p, k), ("--skip-records", c, k), ("--check-ptau", "--verify", k),
                 ("--verify-key", "--name", "x", c, p, k), ("--verify-key", "--lagrange")):
        rc, err = _cli(*args)
        assert rc == 2 and "usage: groth16-contribute" in err and "--verify-key [--lagrange auto|file|compute] [--skip-records] [--check-ptau]" in err, args
    rc, err = _cli("--verify-key", c, p, str(tmp_path / "missing.zkey"))
    assert rc == 2 and "cannot read" in err and "missing.zkey" in err
    rc, err = _cli("--verify-key", str(tmp_path / "missing.r1cs"), p, k)
    assert rc == 2 and "cannot read" in err and "missing.r1cs" in err
    rc, err = _cli("--verify-key", c, p, junk)
    assert rc == 2 and err.startswith("error: zkey")
    rc, err = _cli("--verify-key", k, p, k)
    assert rc == 2 and err.startswith("error: %s: " % k)
    rc, err = _cli("--verify-key", c, k, k)
    assert rc == 2 and err.startswith("error: ptau")
    # the size rule is a verdict, and it comes before the device is touched
    rc, err = _cli("--verify-key", "--skip-records", "--check-ptau", "--lagrange", "auto", c, p, k)
    assert rc == 1 and err.strip() == "INVALID: zkey verify: nVars of the key is 5, the circuit's is 4"
