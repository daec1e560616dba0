"""The Python binding of the C ABI (circom-witnesscalc_amd/_abi.py) without a device: the two declaration tables against
include/*.h, the attribute surface of the package, that importing it does not import torch, and the one call path against a stub."""
import ctypes
import glob
import os
import re
import subprocess
import sys

import pytest

import cwc_import

PKG = cwc_import.load()
ABI = PKG._abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RETURN_TYPES = {"int": ctypes.c_int, "void": None, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
                "double": ctypes.c_double}


def declarations():
    """{name: (return type text, [parameter text])} of every gw_* / gwb_* function that include/*.h declares, comments and
    preprocessor lines stripped"""
    out = {}
    for h in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        txt = open(h).read()
        txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
        txt = re.sub(r"//[^\n]*", " ", txt)
        txt = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", txt, flags=re.M)
        for m in re.finditer(r"([A-Za-z_][A-Za-z_0-9 \t\n\*]*?)\b(gwb?_[a-z_0-9]+)\s*\(([^()]*)\)\s*[;{]", txt):
            ret, name, params = m.groups()
            params = [" ".join(p.split()) for p in params.split(",")]
            assert name not in out, "%s is declared twice" % name
            out[name] = (" ".join(w for w in ret.split() if w not in ("static", "inline", "extern")), [] if params in ([""], ["void"]) else params)
    return out


def is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def test_tables_agree_with_the_headers():
    decl = declarations()
    assert decl.pop("gw_free_status") == ("void", ["gw_status_t *status"])  # header-inline, as in the reference header
    assert len(decl) > 150
    assert not set(ABI.ABI) & set(ABI.R1CS_ABI)
    assert set(decl) == set(ABI.ABI) | set(ABI.R1CS_ABI)
    assert ABI.OPTIONAL <= set(ABI.ABI)
    for name, (ret, params) in decl.items():
        restype, argtypes = (ABI.ABI.get(name) or ABI.R1CS_ABI[name])
        assert len(argtypes) == len(params), name
        if "*" in ret:
            assert restype in (ctypes.c_void_p, ctypes.c_char_p), name
        else:
            assert restype is RETURN_TYPES[ret], name
        for p, t in zip(params, argtypes):
            if "*" in p:
                assert is_pointer(t) and ctypes.sizeof(t) == ctypes.sizeof(ctypes.c_void_p), (name, p)
            elif "size_t" in p.split():
                assert t is ctypes.c_size_t, (name, p)
            else:
                assert not is_pointer(t), (name, p)
        if params and "gw_status_t" in params[-1]:
            assert argtypes[-1] is ABI.stp, name


def test_exported_symbols_are_the_first_table():
    assert PKG.EXPORTED_SYMBOLS == list(ABI.ABI)


# dir() of the package before the binding got its own module, without the double-underscore names
ATTRIBUTES = (
    "CLASS_NAMES", "CONTRIBUTION_HASH_BYTES", "DIAG_LIB_PATH", "E2eStats", "EXPORTED_SYMBOLS", "FORM_CANONICAL",
    "FORM_MONTGOMERY", "G2_CHECK_METHODS", "GROTH16_CONTRIBUTE_PHASES", "GROTH16_CPROOF_BYTES", "GROTH16_PHASES",
    "GROTH16_PROOF_BYTES", "GROTH16_SETUP_PHASES", "GROTH16_SETUP_PTAU_PHASES", "GROTH16_VERIFY_KEY_PHASES", "GT_BYTES",
    "Graph", "GraphInfo", "Groth16", "Groth16VerifyingKey", "GwStatus", "Handoff", "KZG_CHECK_POWERS", "KZG_EQUATION",
    "KZG_PHASES", "KZG_POINT", "KZG_SCALAR", "KZG_VALID", "Kzg", "KzgInfo", "LIB_PATH", "MUL_METHODS", "PTAU_ALL_LEVELS",
    "PTAU_CONTRIBUTE_PHASES", "PTAU_LAGRANGE_MODES", "PTAU_PREPARE_PHASES", "PTAU_RECORD_POINTS", "PTAU_VERIFY_SKIP_RECORDS",
    "ProgramStats", "PtauInfo", "R1CS_LIB_PATH", "R1CS_SATISFIED", "R1cs", "R1csInfo", "R1csQapInfo", "Timing",
    "VERIFY_EQUATION", "VERIFY_KEY_CHECK_PTAU", "VERIFY_KEY_SKIP_RECORDS", "VERIFY_POINT", "VERIFY_PUBLIC",
    "VERIFY_STATUS_NAMES", "VERIFY_SUBGROUP", "VERIFY_VALID", "WitnessCalcError", "ZkeyInfo", "_HERE", "_beacon_call",
    "_beacon_items", "_check", "_codec_args", "_compress_batch_device", "_dec", "_decompress_batch_device", "_from_json_g1",
    "_from_json_g2", "_gt_json", "_int32", "_json_g1", "_json_g2", "_kzg_dev", "_kzg_host", "_kzg_log2", "_lagrange_mode",
    "_lib", "_libc", "_lincomb128_device", "_lincomb_device", "_mul_batch_device", "_pack_schedule", "_ptau_buffer",
    "_public_array", "_qap_batch", "_qap_batch_device", "_qap_info", "_r1cs_check", "_r1cs_lib", "_require_beacon",
    "_rs_array", "_seed32", "_take_image", "_take_status", "beacon_scalars", "bn254_g1_compress_batch_device",
    "bn254_g1_decompress_batch_device", "bn254_g1_lincomb128_device", "bn254_g1_lincomb_device", "bn254_g1_mul_batch_device",
    "bn254_g1_scale_batch_device", "bn254_g2_check_batch_device", "bn254_g2_compress_batch_device",
    "bn254_g2_decompress_batch_device", "bn254_g2_lincomb128_device", "bn254_g2_lincomb_device", "bn254_g2_mul_batch_device",
    "bn254_gen_mul_batch_device", "bn254_pairing_batch_device", "bn254_point_idft_batch_device", "build", "calc_witness",
    "calc_witness_wtns", "ctypes", "graphgen", "graphgen_native", "groth16_beacon", "groth16_compress_proofs",
    "groth16_compress_proofs_device", "groth16_contribute", "groth16_contribute_phase_ms", "groth16_decompress_proofs",
    "groth16_decompress_proofs_device", "groth16_setup", "groth16_setup_phase_ms", "groth16_setup_ptau",
    "groth16_setup_ptau_phase_ms", "groth16_verify_contribution_step", "groth16_verify_contributions", "groth16_verify_key",
    "groth16_verify_key_phase_ms", "kernel_source_hash", "kzg_eval_quotient_device", "kzg_phase_ms", "kzg_tiles", "lib",
    "model_cycles", "modmul_rate", "np", "os", "pack_schedule_of_blob", "pick_tile_width", "pinned_rows", "proof_json",
    "ptau_beacon", "ptau_check", "ptau_check_g2", "ptau_check_lagrange", "ptau_check_powers", "ptau_contribute",
    "ptau_contribute_phase_ms", "ptau_contributions", "ptau_info", "ptau_new", "ptau_prepare_phase2", "ptau_prepare_phase_ms",
    "ptau_verify", "ptau_verify_step", "r1cs_lib", "sha256", "subprocess", "ubench_modmul", "wtns_from_witness",
    "wtns_save_batch", "zkey_contributions",
)


def test_every_earlier_attribute_is_still_there():
    assert len(ATTRIBUTES) == len(set(ATTRIBUTES)) == 163
    assert [n for n in ATTRIBUTES if not hasattr(PKG, n)] == []
    for name in ("GwStatus", "GraphInfo", "Timing", "ProgramStats", "E2eStats", "Handoff", "R1csInfo", "R1csQapInfo", "ZkeyInfo", "PtauInfo", "KzgInfo",
                 "WitnessCalcError", "LIB_PATH", "DIAG_LIB_PATH", "R1CS_LIB_PATH", "lib", "r1cs_lib", "_libc"):
        assert getattr(PKG, name) is getattr(ABI, name), name
    # the loaded libraries live in _abi; the package shows the same objects, before and after the first use
    assert PKG._lib is ABI._lib and PKG._r1cs_lib is ABI._r1cs_lib
    assert PKG.lib() is PKG._lib is ABI._lib and PKG.r1cs_lib() is PKG._r1cs_lib is ABI._r1cs_lib


def test_both_tables_apply_to_the_built_libraries():
    for L, table in ((PKG.lib(), ABI.ABI), (PKG.r1cs_lib(), ABI.R1CS_ABI)):
        for name, (restype, argtypes) in table.items():
            f = getattr(L, name)
            assert f.restype is restype and list(f.argtypes) == argtypes, name


def test_import_does_not_import_torch():
    code = "import sys; import cwc_import; cwc_import.load(); assert 'torch' not in sys.modules, 'torch was imported'"
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


# -- the call path against a stub ----------------------------------------------------------------------------------------------------
class Stub:
    """a C function as the call path sees one: fills the status it is handed, from a buffer the test owns, and returns rc"""

    def __init__(self, rc, message):
        self.rc, self.buf, self.args = rc, None if message is None else ctypes.create_string_buffer(message), None
        self.freed = []

    def __call__(self, *args):
        st = args[-1]._obj
        assert isinstance(st, PKG.GwStatus)
        st.code = self.rc
        st.error_msg = None if self.buf is None else ctypes.addressof(self.buf)
        self.args = args[:-1]
        return self.rc

    def free(self, st):
        self.freed.append(st.error_msg)


def test_call_passes_its_arguments_and_returns_quietly():
    f = Stub(0, None)
    assert ABI.call(f.free, f, 1, b"two", None) is None
    assert f.args == (1, b"two", None) and f.freed == []


def test_call_raises_with_the_message_and_frees_it_once():
    f = Stub(1, b"boom")
    with pytest.raises(PKG.WitnessCalcError) as e:
        ABI.call(f.free, f, 7)
    assert str(e.value) == "boom" and f.args == (7,)
    assert f.freed == [ctypes.addressof(f.buf)]


def test_call_without_a_message_says_call_failed():
    f = Stub(2, None)
    with pytest.raises(PKG.WitnessCalcError) as e:
        ABI.call(f.free, f)
    assert str(e.value) == "call failed" and f.freed == []


def test_call_frees_the_message_of_a_call_that_succeeded():
    f = Stub(0, b"a note")
    ABI.call(f.free, f)
    assert f.freed == [ctypes.addressof(f.buf)]


def test_package_call_paths_are_bound_to_their_library_rule():
    assert PKG._call.func is ABI.call and PKG._call.args == (ABI.free_status,)
    assert PKG._r1cs_call.func is ABI.call and PKG._r1cs_call.args == (ABI.free_malloced,)
