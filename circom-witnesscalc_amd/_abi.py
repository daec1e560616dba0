"""The C ABI as ctypes sees it: the structures of include/*.h, one declaration table per shared library, the two lazy loaders
that apply them, and the one call path of every function that reports through a gw_status_t.

A new C function is declared here, by one line in its library's table (ABI for libcircom_witnesscalc_amd.so, R1CS_ABI for
libcwc_r1cs.so): name -> (return type, argument types).  tests/test_python_abi_host.py holds both tables against the headers."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CWC_LIB_PATH") or os.path.join(_HERE, "libcircom_witnesscalc_amd.so")
DIAG_LIB_PATH = os.path.join(_HERE, "libcircom_witnesscalc_amd_diag.so")
R1CS_LIB_PATH = os.environ.get("CWC_R1CS_LIB_PATH") or os.path.join(_HERE, "libcwc_r1cs.so")
_lib = None
_r1cs_lib = None


class GwStatus(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int), ("error_msg", ctypes.c_void_p)]


class GraphInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_nodes", "n_op", "n_input_nodes", "n_const", "n_inputs",
                                                "n_witness", "depth", "algorithmic_bytes_per_set")]


class Timing(ctypes.Structure):
    _fields_ = [("tile_width", ctypes.c_uint32), ("n_launches", ctypes.c_uint32), ("n_bundles", ctypes.c_uint64),
                ("n_slots", ctypes.c_uint64), ("interp_ms", ctypes.c_float), ("pack_ms", ctypes.c_float),
                ("divider", ctypes.c_uint32), ("streams", ctypes.c_uint32)]


class ProgramStats(ctypes.Structure):
    _fields_ = [("tile_width", ctypes.c_uint32), ("divider", ctypes.c_uint32), ("streams", ctypes.c_uint32), ("n_classes", ctypes.c_uint32),
                ("n_bundles", ctypes.c_uint64), ("n_fused_nodes", ctypes.c_uint64), ("class_bundles", ctypes.c_uint64 * 16),
                ("class_nodes", ctypes.c_uint64 * 16), ("model_wave_cycles", ctypes.c_double), ("lanes_active_mean", ctypes.c_double),
                ("values_per_bundle_mean", ctypes.c_double), ("chain_floor_cycles", ctypes.c_double), ("n_scan_steps", ctypes.c_uint64), ("n_conv_products", ctypes.c_uint64)]


class E2eStats(ctypes.Structure):
    _fields_ = [("n_sets", ctypes.c_size_t), ("sub_batch", ctypes.c_size_t), ("parse_threads", ctypes.c_uint32), ("write_threads", ctypes.c_uint32),
                ("parse_seconds", ctypes.c_double), ("wait_for_drain_seconds", ctypes.c_double), ("total_seconds", ctypes.c_double),
                ("witness_bytes", ctypes.c_uint64), ("failed_sets", ctypes.c_uint64)]


class Handoff(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("form", ctypes.c_uint32), ("hip_stream", ctypes.c_void_p), ("done_event", ctypes.c_void_p)]


class R1csInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("n_wires", "n_pub_out", "n_pub_in", "n_prv_in", "n_constraints")] + \
               [(n, ctypes.c_uint64) for n in ("n_labels", "n_factors_a", "n_factors_b", "n_factors_c")]


class R1csQapInfo(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_uint64), ("domain_power", ctypes.c_uint32), ("domain_size", ctypes.c_uint64),
                ("workspace_bytes_per_row", ctypes.c_uint64)]


class ZkeyInfo(ctypes.Structure):
    _fields_ = [("n_vars", ctypes.c_uint32), ("n_public", ctypes.c_uint32), ("domain_size", ctypes.c_uint32), ("n_coefs", ctypes.c_uint64)]


class PtauInfo(ctypes.Structure):
    _fields_ = [("power", ctypes.c_uint32), ("ceremony_power", ctypes.c_uint32), ("prepared", ctypes.c_uint32),
                ("n_contributions", ctypes.c_uint32)]


class KzgInfo(ctypes.Structure):
    _fields_ = [("max_len", ctypes.c_uint64), ("power", ctypes.c_uint32), ("prepared", ctypes.c_uint32)]


class WitnessCalcError(RuntimeError):
    pass


# -- the declaration tables ------------------------------------------------------------------------------------------------------
P = ctypes.POINTER
vp, cstr, sz, i32, u32, u64, f32, f64 = (ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64,
                                        ctypes.c_float, ctypes.c_double)
stp = P(GwStatus)

# include/graph_witness.h and include/graph_witness_batch.h (libcircom_witnesscalc_amd.so); the keys are EXPORTED_SYMBOLS
ABI = {
    "gw_calc_witness": (i32, [cstr, vp, sz, P(vp), P(sz), stp]),
    "gwb_graph_load": (i32, [vp, sz, P(vp), stp]),
    "gwb_graph_free": (None, [vp]),
    "gwb_graph_info": (i32, [vp, P(GraphInfo)]),
    "gwb_graph_serialize": (i32, [vp, P(vp), P(sz), stp]),
    "gwb_builder_new": (vp, []),
    "gwb_builder_free": (None, [vp]),
    "gwb_builder_input": (u32, [vp, u32]),
    "gwb_builder_constant": (u32, [vp, cstr, sz]),
    "gwb_builder_uno": (u32, [vp, u32, u32]),
    "gwb_builder_duo": (u32, [vp, u32, u32, u32]),
    "gwb_builder_tres": (u32, [vp, u32, u32, u32, u32]),
    "gwb_builder_witness": (i32, [vp, u32]),
    "gwb_builder_input_signal": (i32, [vp, cstr, u32, u32]),
    "gwb_builder_node_count": (u64, [vp]),
    "gwb_builder_finish": (i32, [vp, P(vp), P(sz), stp]),
    "gwb_graphgen_bigint_class": (i32, [u32, u32, u32, P(vp), P(sz), stp]),
    "gwb_graphgen_rsa_long_div_class": (i32, [u32, u32, u32, i32, P(vp), P(sz), stp]),
    "gwb_graph_op_histogram": (i32, [vp, P(u64), sz]),
    "gwb_inputs_from_json": (i32, [vp, cstr, vp, stp]),
    "gwb_inputs_from_json_batch": (i32, [vp, cstr, sz, vp, sz, P(sz), stp]),
    "gwb_wtns_save_batch": (i32, [vp, sz, sz, cstr, stp]),
    "gwb_calc_witness_json_to_wtns": (i32, [vp, cstr, sz, cstr, sz, P(sz), vp, sz, P(E2eStats), stp]),
    "gwb_set_tile_width": (i32, [vp, u32]),
    "gwb_pick_tile_width": (u32, [sz]),
    "gwb_graph_pick_tile_width": (u32, [vp, sz]),
    "gwb_calc_witness_batch_device": (i32, [vp, vp, sz, vp, vp, vp, stp]),
    "gwb_calc_witness_batch_handoff": (i32, [vp, vp, sz, vp, vp, P(Handoff), stp]),
    "gwb_calc_witness_batch_host": (i32, [vp, vp, sz, vp, vp, stp]),
    "gwb_host_alloc": (vp, [sz]),
    "gwb_host_free": (None, [vp]),
    "gwb_last_timing": (i32, [vp, P(Timing)]),
    "gwb_timing_history": (i32, [vp, sz, vp, vp, P(sz)]),
    "gwb_profile_classes": (i32, [vp, vp, sz, vp, vp, vp, stp]),
    "gwb_wave_census": (i32, [vp, vp, sz, vp, vp, vp, sz, stp]),
    "gwb_ubench_modmul": (f64, [u32, u32]),
    "gwb_ubench_modmul_block": (f64, [u32, u32]),
    "gwb_model_class_cycles": (f64, [u32]),
    "gwb_kernel_source_hash": (cstr, []),
    "gwb_program_stats": (i32, [vp, u32, P(ProgramStats)]),
    "gwb_pack_schedule": (i32, [vp, u32, vp, sz, vp, sz, P(u32), P(u32), P(u32), stp]),
    "gwb_pack_schedule_of_blob": (i32, [vp, sz, vp, sz, vp, sz, P(u32), P(u32), P(u32), stp]),
    "gwb_wtns_size": (sz, [sz]),
    "gwb_wtns_from_witness": (i32, [vp, sz, vp]),
    "gwb_graph_export": (i32, [vp, u32, P(vp), P(sz), stp]),
    "gwb_graph_import": (i32, [vp, sz, P(vp), stp]),
    "gwb_rccl_unique_id": (i32, [vp, stp]),
    "gwb_rccl_comm_init": (i32, [vp, i32, i32, P(vp), stp]),
    "gwb_rccl_comm_ranks": (i32, [vp]),
    "gwb_rccl_comm_destroy": (None, [vp]),
    "gwb_graph_broadcast": (i32, [vp, u32, sz, i32, i32, vp, vp, P(vp), stp]),
    "gwb_free_status": (None, [stp]),
}

# A library may lack these and still load (absent from an older build loaded through CWC_LIB_PATH for a same-box A/B); every other
# symbol of either table is required, and a library without it fails at load.
OPTIONAL = frozenset(("gwb_graphgen_bigint_class", "gwb_graphgen_rsa_long_div_class", "gwb_graph_op_histogram", "gwb_wave_census",
                      "gwb_pack_schedule", "gwb_pack_schedule_of_blob"))

# every other header of include/ (libcwc_r1cs.so)
R1CS_ABI = {
    # graph_witness_r1cs.h
    "gwb_r1cs_load": (i32, [vp, sz, P(vp), stp]),
    "gwb_r1cs_free": (None, [vp]),
    "gwb_r1cs_info": (i32, [vp, P(R1csInfo)]),
    "gwb_r1cs_set_tile_width": (i32, [vp, u32]),
    "gwb_r1cs_check_batch_device": (i32, [vp, vp, sz, sz, u32, vp, vp, vp, stp]),
    "gwb_r1cs_check_batch_host": (i32, [vp, vp, sz, sz, vp, vp, stp]),
    "gwb_r1cs_check_wtns": (i32, [vp, vp, sz, vp, vp, stp]),
    "gwb_r1cs_qap_info": (i32, [vp, P(R1csQapInfo), stp]),
    "gwb_r1cs_qap_batch_device": (i32, [vp, vp, sz, sz, u32, vp, u32, vp, stp]),
    "gwb_r1cs_qap_batch_host": (i32, [vp, vp, sz, sz, vp, u32, stp]),
    "gwb_r1cs_qap_wtns": (i32, [vp, vp, sz, vp, u32, stp]),
    "gwb_r1cs_qap_time_phases": (i32, [vp, i32]),
    "gwb_r1cs_qap_phase_ms": (i32, [vp, P(f32)]),
    "gwb_r1cs_modmul_rate": (i32, [P(f64)]),
    # graph_witness_groth16.h
    "gwb_zkey_load": (i32, [vp, sz, P(vp), stp]),
    "gwb_zkey_free": (None, [vp]),
    "gwb_zkey_info": (i32, [vp, P(ZkeyInfo)]),
    "gwb_groth16_prove_batch_device": (i32, [vp, vp, vp, sz, sz, u32, vp, vp, vp, stp]),
    "gwb_groth16_prove_batch_host": (i32, [vp, vp, vp, sz, sz, vp, vp, stp]),
    "gwb_groth16_prove_wtns": (i32, [vp, vp, vp, sz, vp, vp, stp]),
    "gwb_groth16_time_phases": (i32, [vp, i32]),
    "gwb_groth16_phase_ms": (i32, [vp, P(f32)]),
    "gwb_zkey_qap_info": (i32, [vp, P(R1csQapInfo), stp]),
    "gwb_zkey_qap_batch_device": (i32, [vp, vp, sz, sz, u32, vp, u32, vp, stp]),
    "gwb_zkey_qap_batch_host": (i32, [vp, vp, sz, sz, vp, u32, stp]),
    "gwb_zkey_set_tile_width": (i32, [vp, u32]),
    "gwb_zkey_check_r1cs": (i32, [vp, vp, stp]),
    "gwb_zkey_check_g2": (i32, [vp, stp]),
    "gwb_zkey_check_wtns": (i32, [vp, vp, sz, stp]),
    # graph_witness_groth16_verify.h
    "gwb_g16vk_from_zkey": (i32, [vp, P(vp), stp]),
    "gwb_g16vk_load": (i32, [vp, sz, u32, P(vp), stp]),
    "gwb_g16vk_info": (i32, [vp, P(u32)]),
    "gwb_g16vk_points": (i32, [vp, vp, sz]),
    "gwb_g16vk_alphabeta": (i32, [vp, vp, stp]),
    "gwb_g16vk_free": (None, [vp]),
    "gwb_groth16_verify_batch_device": (i32, [vp, vp, vp, sz, sz, vp, vp, stp]),
    "gwb_groth16_verify_batch_host": (i32, [vp, vp, vp, sz, sz, vp, stp]),
    "gwb_bn254_pairing_batch_device": (i32, [vp, vp, sz, vp, vp, stp]),
    "gwb_bn254_g2_check_batch_device": (i32, [vp, sz, u32, u32, vp, vp, stp]),
    # graph_witness_groth16_setup.h
    "gwb_groth16_setup": (i32, [vp, vp, P(vp), P(sz), stp]),
    "gwb_groth16_setup_free": (None, [vp]),
    "gwb_bn254_gen_mul_batch_device": (i32, [vp, sz, u32, vp, vp, stp]),
    "gwb_groth16_setup_phase_ms": (i32, [P(f32)]),
    # graph_witness_groth16_ptau.h
    "gwb_ptau_info": (i32, [vp, sz, P(PtauInfo), stp]),
    "gwb_ptau_check": (i32, [vp, sz, u32, u32, stp]),
    "gwb_ptau_check_g2": (i32, [vp, sz, u32, u32, stp]),
    "gwb_ptau_check_powers": (i32, [vp, sz, u32, vp, stp]),
    "gwb_ptau_prepare_phase2": (i32, [vp, sz, P(vp), P(sz), stp]),
    "gwb_ptau_prepare_phase_ms": (i32, [P(f32)]),
    "gwb_ptau_check_lagrange": (i32, [vp, sz, u32, vp, stp]),
    "gwb_bn254_g1_lincomb_device": (i32, [vp, vp, sz, u32, vp, vp, stp]),
    "gwb_bn254_g2_lincomb_device": (i32, [vp, vp, sz, u32, vp, vp, stp]),
    "gwb_groth16_setup_ptau": (i32, [vp, vp, sz, vp, u32, P(vp), P(sz), stp]),
    "gwb_bn254_point_idft_batch_device": (i32, [vp, u32, u32, vp, vp, stp]),
    "gwb_groth16_setup_ptau_phase_ms": (i32, [P(f32)]),
    # graph_witness_groth16_contribute.h
    "gwb_groth16_contribute": (i32, [vp, sz, cstr, vp, P(vp), P(sz), vp, stp]),
    "gwb_groth16_contribute_phase_ms": (i32, [P(f32)]),
    "gwb_zkey_verify_contributions": (i32, [vp, sz, vp, P(sz), stp]),
    "gwb_zkey_verify_step": (i32, [vp, sz, vp, sz, vp, stp]),
    "gwb_zkey_verify_key": (i32, [vp, sz, vp, vp, sz, u32, u32, vp, vp, P(sz), stp]),
    "gwb_zkey_verify_key_phase_ms": (i32, [P(f32)]),
    "gwb_zkey_contributions": (i32, [vp, sz, P(vp), P(sz), stp]),
    "gwb_blake2b512": (None, [vp, sz, vp]),
    "gwb_zkey_contribution_challenge": (None, [vp, vp]),
    "gwb_bn254_g1_scale_batch_device": (i32, [vp, sz, vp, vp, vp, stp]),
    "gwb_bn254_g1_lincomb128_device": (i32, [vp, vp, sz, vp, vp, stp]),
    "gwb_bn254_g2_lincomb128_device": (i32, [vp, vp, sz, vp, vp, stp]),
    # graph_witness_groth16_ceremony.h
    "gwb_ptau_new": (i32, [u32, P(vp), P(sz), stp]),
    "gwb_ptau_contribute": (i32, [vp, sz, cstr, vp, P(vp), P(sz), vp, stp]),
    "gwb_ptau_contribute_phase_ms": (i32, [P(f32)]),
    "gwb_ptau_verify": (i32, [vp, sz, u32, vp, vp, P(sz), stp]),
    "gwb_ptau_verify_step": (i32, [vp, sz, vp, sz, vp, stp]),
    "gwb_ptau_contributions": (i32, [vp, sz, P(vp), P(sz), stp]),
    "gwb_bn254_g1_mul_batch_device": (i32, [vp, vp, sz, u32, u32, vp, vp, stp]),
    "gwb_bn254_g2_mul_batch_device": (i32, [vp, vp, sz, u32, u32, vp, vp, stp]),
    # graph_witness_groth16_beacon.h
    "gwb_ptau_beacon": (i32, [vp, sz, cstr, vp, sz, u32, P(vp), P(sz), vp, stp]),
    "gwb_groth16_beacon": (i32, [vp, sz, cstr, vp, sz, u32, P(vp), P(sz), vp, stp]),
    "gwb_beacon_scalars": (i32, [u32, vp, sz, u32, vp]),
    "gwb_ptau_contribution_params": (i32, [vp, sz, sz, P(vp), P(sz), stp]),
    "gwb_zkey_contribution_params": (i32, [vp, sz, sz, P(vp), P(sz), stp]),
    "gwb_sha256": (None, [vp, sz, vp]),
    # graph_witness_groth16_compressed.h
    "gwb_bn254_compress_batch_device": (i32, [vp, sz, u32, u32, vp, vp, stp]),
    "gwb_bn254_decompress_batch_device": (i32, [vp, sz, u32, u32, vp, vp, vp, stp]),
    "gwb_groth16_proofs_compress_device": (i32, [vp, sz, vp, vp, stp]),
    "gwb_groth16_proofs_decompress_device": (i32, [vp, sz, vp, vp, vp, stp]),
    "gwb_groth16_verify_batch_compressed_device": (i32, [vp, vp, vp, sz, sz, vp, vp, stp]),
    "gwb_groth16_verify_batch_compressed_host": (i32, [vp, vp, vp, sz, sz, vp, stp]),
    "gwb_g16vk_load_compressed": (i32, [vp, sz, P(vp), stp]),
    "gwb_g16vk_compressed": (i32, [vp, vp, sz]),
    # graph_witness_kzg.h
    "gwb_kzg_new": (i32, [vp, sz, u64, u32, P(vp), stp]),
    "gwb_kzg_info": (i32, [vp, P(KzgInfo)]),
    "gwb_kzg_free": (None, [vp]),
    "gwb_kzg_commit_batch": (i32, [vp, vp, sz, sz, vp, stp]),
    "gwb_kzg_commit_batch_device": (i32, [vp, vp, sz, sz, vp, vp, stp]),
    "gwb_kzg_commit_evals_batch": (i32, [vp, vp, sz, u32, vp, stp]),
    "gwb_kzg_commit_evals_batch_device": (i32, [vp, vp, sz, u32, vp, vp, stp]),
    "gwb_kzg_eval_batch": (i32, [vp, vp, vp, sz, sz, vp, stp]),
    "gwb_kzg_eval_batch_device": (i32, [vp, vp, vp, sz, sz, vp, vp, stp]),
    "gwb_kzg_open_batch": (i32, [vp, vp, vp, sz, sz, vp, vp, stp]),
    "gwb_kzg_open_batch_device": (i32, [vp, vp, vp, sz, sz, vp, vp, vp, stp]),
    "gwb_kzg_verify_batch": (i32, [vp, vp, vp, vp, vp, sz, vp, stp]),
    "gwb_kzg_verify_batch_device": (i32, [vp, vp, vp, vp, vp, sz, vp, vp, stp]),
    "gwb_kzg_phase_ms": (i32, [vp, P(f32)]),
    "gwb_kzg_eval_quotient_device": (i32, [vp, vp, sz, sz, u32, vp, vp, vp, stp]),
    "gwb_kzg_tiles": (i32, [P(u32), P(sz)]),
    "gwb_kzg_open_fold_batch": (i32, [vp, vp, vp, vp, sz, sz, sz, vp, vp, stp]),
    "gwb_kzg_open_fold_batch_device": (i32, [vp, vp, vp, vp, sz, sz, sz, vp, vp, vp, stp]),
    "gwb_kzg_verify_fold_batch": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, vp, stp]),
    "gwb_kzg_verify_fold_batch_device": (i32, [vp, vp, vp, vp, vp, vp, sz, sz, vp, vp, stp]),
    "gwb_kzg_fold_phase_ms": (i32, [vp, P(f32)]),
    "gwb_kzg_fold_device": (i32, [vp, vp, sz, sz, sz, vp, vp, stp]),
    "gwb_kzg_fold_points_device": (i32, [vp, vp, sz, sz, vp, vp, stp]),
}


# -- the loaders -----------------------------------------------------------------------------------------------------------------
def _load(path, table, missing):
    if not os.path.exists(path):
        raise WitnessCalcError(missing % path)
    # One HIP runtime per process: torch bundles its own libamdhip64 (soname libamdhip64.so.7).  Loading
    # torch first makes this library's NEEDED libamdhip64.so.7 resolve to that already-loaded copy; the
    # other order would map a second runtime (system ROCm) next to torch's and torch then sees no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(path)
    for name, (restype, argtypes) in table.items():
        if name in OPTIONAL and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    return L


def lib():
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH, ABI, "HIP extension %s is missing: run __graft_entry__.build() (there is no CPU fallback)")
    return _lib


def r1cs_lib():
    """ctypes handle of libcwc_r1cs.so, loaded after torch (one HIP runtime per process, as in lib())."""
    global _r1cs_lib
    if _r1cs_lib is None:
        _r1cs_lib = _load(R1CS_LIB_PATH, R1CS_ABI, "R1CS library %s is missing: run __graft_entry__.build()")
    return _r1cs_lib


# -- the call path ---------------------------------------------------------------------------------------------------------------
_libc = ctypes.CDLL(None)
_libc.free.argtypes = [ctypes.c_void_p]


def free_status(st):
    """how a message of libcircom_witnesscalc_amd.so is freed"""
    lib().gwb_free_status(ctypes.byref(st))


def free_malloced(st):
    """how a message of libcwc_r1cs.so is freed"""
    _libc.free(st.error_msg)


def take_message(free, st):
    """the message of a status ("" when it has none), freed by its library's rule `free`"""
    if not st.error_msg:
        return ""
    msg = ctypes.string_at(st.error_msg).decode("utf-8", "replace")
    free(st)
    return msg


def check(free, rc, st):
    msg = take_message(free, st)
    if rc != 0:
        raise WitnessCalcError(msg or "call failed")


def call(free, fn, *args):
    """fn(*args, &status) for a C function whose last parameter is its gw_status_t*; raises WitnessCalcError with the status's
    message on a non-zero return"""
    st = GwStatus()
    check(free, fn(*args, ctypes.byref(st)), st)
