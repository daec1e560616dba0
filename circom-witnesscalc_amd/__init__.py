"""MI355X-native calc-witness path of circom-witnesscalc -- Python host-side mirror of the C-ABI.

The product is `libcircom_witnesscalc_amd.so` (HIP kernels for gfx950 + C++ host, see csrc/ and
include/*.h).  This module binds it with ctypes and mirrors the reference's Rust-level API names
(reference src/lib.rs:114-247): `calc_witness`, `wtns_from_witness`, `deserialize_inputs`-equivalent
`inputs_from_json`, plus the additive batch API.  torch is used only to hold device buffers.

There is no CPU evaluation path: every witness value is computed by the HIP kernels; without the
shared library or without a HIP device the calls raise.
"""
import contextlib
import ctypes
import functools
import os
import subprocess

import numpy as np

from . import _abi
from ._abi import (DIAG_LIB_PATH, LIB_PATH, R1CS_LIB_PATH, E2eStats, GraphInfo, GwStatus, Handoff, KzgInfo,  # noqa: F401
                   ProgramStats, PtauInfo, R1csInfo, R1csQapInfo, Timing, WitnessCalcError, ZkeyInfo, _HERE, _libc, lib, r1cs_lib)

CLASS_NAMES = ["INPUT", "MUL", "LIN", "DIV", "CMPZ", "CMPS", "BIT", "IDIVMOD", "TERN", "DIVREQ", "DIVGET", "MULQ", "SYNC", "MULF", "SCAN"]
FORM_CANONICAL, FORM_MONTGOMERY = 0, 1
EXPORTED_SYMBOLS = list(_abi.ABI)

# The one call path, bound to each library's rule for freeing a status message: _call for lib(), _r1cs_call for r1cs_lib().
# The other three take a status that the caller made (callers of the raw C functions outside this module).
_call = functools.partial(_abi.call, _abi.free_status)
_r1cs_call = functools.partial(_abi.call, _abi.free_malloced)
_check = functools.partial(_abi.check, _abi.free_status)
_r1cs_check = functools.partial(_abi.check, _abi.free_malloced)
_take_status = functools.partial(_abi.take_message, _abi.free_status)


def __getattr__(name):
    """_lib and _r1cs_lib: the loaded libraries, None before their first use (they live in _abi, which rebinds them)"""
    if name in ("_lib", "_r1cs_lib"):
        return getattr(_abi, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def _form(montgomery):
    return FORM_MONTGOMERY if montgomery else FORM_CANONICAL


def _take_image(out, n, free=None):
    """the bytes of a malloc'ed image that a call handed out, which is then freed (by gwb_groth16_setup_free unless told otherwise)"""
    try:
        return ctypes.string_at(out, n.value)
    finally:
        (free or r1cs_lib().gwb_groth16_setup_free)(out)


class _Handle:
    """close() and __del__ of a class that owns a C handle in self._h.  _FREE: (the name under which _abi holds the loaded
    library, the handle's free function).  The library is read, never loaded here, and a handle is only freed while it is still
    there: that makes __del__ safe at interpreter shutdown."""
    _FREE = None

    def close(self):
        L = getattr(_abi, self._FREE[0], None)
        if getattr(self, "_h", None) and L is not None:
            getattr(L, self._FREE[1])(self._h)
            self._h = None

    __del__ = close


def _stream_of(t, stream):
    import torch
    return stream if stream is not None else torch.cuda.current_stream(t.device)


@contextlib.contextmanager
def _device_call(t, stream, record=()):
    """The skeleton of an asynchronous device call: yields `stream`, or the current stream of t's device, with that device
    current for the call inside; afterwards the tensors of `record` that have elements are recorded on the stream (so the
    caching allocator keeps their memory until the call's work is done).  Nothing is recorded when the call raises."""
    import torch
    s = _stream_of(t, stream)
    with torch.cuda.device(t.device):
        yield s
    for x in record:
        if x.numel():
            x.record_stream(s)


def _phase_ms(fn, names, what, handle=None):
    ms = (ctypes.c_float * len(names))()
    if fn(*(() if handle is None else (handle,)), ms) != 0:
        raise WitnessCalcError(what)
    return dict(zip(names, (float(x) for x in ms)))


def _name_bytes(name):
    nm = name.encode("utf-8") if isinstance(name, str) else bytes(name)
    if b"\0" in nm:
        raise WitnessCalcError("the name holds a zero byte")
    return nm


@contextlib.contextmanager
def _secret_scalars(values, refusals):
    """None for None; else the ints as 32 little-endian bytes each in one ctypes buffer, zeroed on the way out.  refusals[i] is
    the caller's message for values[i] outside [0, 2^256)."""
    if values is None:
        yield None
        return
    for v, refusal in zip(values, refusals):
        if not 0 <= v < (1 << 256):
            raise WitnessCalcError(refusal)
    buf = ctypes.create_string_buffer(b"".join(v.to_bytes(32, "little") for v in values), 32 * len(values))
    try:
        yield buf
    finally:
        ctypes.memset(buf, 0, len(buf))


def pinned_rows(shape):
    """uint8 array in pinned host memory (gwb_host_alloc); freed when the array and its views are gone."""
    import weakref
    n = int(np.prod(shape))
    ptr = lib().gwb_host_alloc(n)
    if not ptr:
        raise WitnessCalcError("gwb_host_alloc(%d) failed" % n)
    buf = (ctypes.c_uint8 * max(n, 1)).from_address(ptr)
    weakref.finalize(buf, lib().gwb_host_free, ptr)
    return np.frombuffer(buf, dtype=np.uint8, count=n).reshape(shape)


def build(verbose=False, diag=False):
    """Compile the HIP extension in-tree (hipcc --offload-arch=gfx950).  diag=True also builds the diagnostic library
    (stamped interpreter instances for gwb_profile_classes; the class-profile / calibration tools load it via CWC_LIB_PATH)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j4"] + (["all", "diag"] if diag else [])
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    # the R1CS check, QAP witness map and Groth16 layers (libcwc_r1cs.so and its CLIs): a library of its own, outside csrc/
    subprocess.check_call(["make"] + ([] if verbose else ["-s"]) + ["-C", os.path.join(_HERE, "r1cs"), "-j4"])


def wtns_save_batch(witness, path_pattern):
    """One `.wtns` file per input set; witness uint8 [B, W, 32]; path_pattern with one %lu (gwb_wtns_save_batch)."""
    witness = np.ascontiguousarray(witness, dtype=np.uint8)
    _call(lib().gwb_wtns_save_batch, witness.ctypes.data, witness.shape[1], witness.shape[0], path_pattern.encode())


def ubench_modmul(waves_per_simd=4, iters=2000, block=False):
    """Chip-wide one-lane Montgomery products per second (gwb_ubench_modmul; block: the interpreter's own multiplier,
    gwb_ubench_modmul_block, at most two waves per SIMD)."""
    if block:
        return float(lib().gwb_ubench_modmul_block(waves_per_simd, iters))
    return float(lib().gwb_ubench_modmul(waves_per_simd, iters))


def kernel_source_hash():
    """SHA-256 of the kernel sources the loaded library's device code was built from (gwb_kernel_source_hash)."""
    return lib().gwb_kernel_source_hash().decode()


def model_cycles():
    """The cost model's lone-wave cycles per bundle class as the library loaded them ({class name: cycles};
    gwb_model_class_cycles): built-in, CWC_MODEL_CYCLES, or the calibration file of tools/gpu_calibrate.py."""
    return {n: float(lib().gwb_model_class_cycles(c)) for c, n in enumerate(CLASS_NAMES)}


def graphgen_native(kind, **kw):
    """`.bin` bytes of one of BASELINE config 5's class graphs from the native generators (gwb_graphgen_*): kind "bigint" (k, n_bits,
    rounds) or "rsa" (n, k, muls, range_checks) -- the same bytes as graphgen.circuits.build_bigint_class / build_rsa_long_div_class
    write, without ten million nodes passing through Python."""
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    L = lib()
    if kind == "bigint":
        _call(L.gwb_graphgen_bigint_class, int(kw.get("k", 8)), int(kw.get("n_bits", 64)), int(kw.get("rounds", 4)), ctypes.byref(out), ctypes.byref(n))
    elif kind == "rsa":
        _call(L.gwb_graphgen_rsa_long_div_class, int(kw.get("n", 121)), int(kw.get("k", 17)), int(kw.get("muls", 2)), 1 if kw.get("range_checks", True) else 0,
              ctypes.byref(out), ctypes.byref(n))
    else:
        raise ValueError(kind)
    return _take_image(out, n, _libc.free)


def pick_tile_width(batch):
    """Input sets per wavefront the library uses for a batch of this size (gwb_pick_tile_width)."""
    return int(lib().gwb_pick_tile_width(batch))


def calc_witness_wtns(inputs_json, graph_data):
    """gw_calc_witness (reference src/lib.rs:44-111): JSON text + `.bin` bytes -> `.wtns` bytes."""
    if isinstance(inputs_json, str):
        inputs_json = inputs_json.encode("utf-8")
    graph_data = bytes(graph_data)
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    _call(lib().gw_calc_witness, inputs_json, graph_data, len(graph_data), ctypes.byref(out), ctypes.byref(n))
    return _take_image(out, n, _libc.free)


def calc_witness(inputs_json, graph_data):
    """calc_witness (reference src/lib.rs:125-136): -> list[int] witness values."""
    w = calc_witness_wtns(inputs_json, graph_data)
    body = w[76:]
    return [int.from_bytes(body[i:i + 32], "little") for i in range(0, len(body), 32)]


def wtns_from_witness(witness):
    """wtns_from_witness (reference src/lib.rs:114-123). witness: list[int] or uint8 array [W, 32]."""
    if not isinstance(witness, np.ndarray):
        witness = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in witness), dtype=np.uint8)
    witness = np.ascontiguousarray(witness, dtype=np.uint8).reshape(-1, 32)
    n = witness.shape[0]
    out = np.zeros(lib().gwb_wtns_size(n), dtype=np.uint8)
    if lib().gwb_wtns_from_witness(witness.ctypes.data, n, out.ctypes.data) != 0:
        raise WitnessCalcError("gwb_wtns_from_witness failed")
    return out.tobytes()


class Graph(_Handle):
    """A parsed + compiled graph (deserialize_witnesscalc_graph, reference src/storage.rs:214-249), reusable
    across calls -- the reference re-parses the `.bin` on every calc_witness (src/lib.rs:129)."""
    _FREE = ("_lib", "gwb_graph_free")

    def __init__(self, graph_data=None, _handle=None):
        self._h = ctypes.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            graph_data = bytes(graph_data)
            _call(lib().gwb_graph_load, graph_data, len(graph_data), ctypes.byref(self._h))
        info = GraphInfo()
        lib().gwb_graph_info(self._h, ctypes.byref(info))
        for name, _ in GraphInfo._fields_:
            setattr(self, name, int(getattr(info, name)))

    @classmethod
    def from_blob(cls, blob):
        """gwb_graph_import: build a replica from a compiled-program blob (what ranks receive over RCCL)."""
        blob = bytes(blob)
        h = ctypes.c_void_p()
        _call(lib().gwb_graph_import, blob, len(blob), ctypes.byref(h))
        return cls(_handle=h)

    def op_histogram(self):
        """{operation name: nodes} of the graph as loaded (gwb_graph_op_histogram)"""
        h = (ctypes.c_uint64 * 24)()
        if lib().gwb_graph_op_histogram(self._h, h, 24) != 0:
            raise WitnessCalcError("gwb_graph_op_histogram failed")
        names = ["Mul", "Div", "Add", "Sub", "Pow", "Idiv", "Mod", "Eq", "Neq", "Lt", "Gt", "Leq", "Geq", "Land", "Lor", "Shl", "Shr", "Bor", "Band", "Bxor",
                 "Neg", "TernCond", "Input", "Const"]
        return dict(sorted(((nm, int(h[i])) for i, nm in enumerate(names) if h[i]), key=lambda kv: -kv[1]))

    def export_blob(self, tile_width):
        out, n = ctypes.c_void_p(), ctypes.c_size_t()
        _call(lib().gwb_graph_export, self._h, tile_width, ctypes.byref(out), ctypes.byref(n))
        return _take_image(out, n, _libc.free)

    def serialize(self):
        """serialize_witnesscalc_graph (reference src/storage.rs:137-183)."""
        out, n = ctypes.c_void_p(), ctypes.c_size_t()
        _call(lib().gwb_graph_serialize, self._h, ctypes.byref(out), ctypes.byref(n))
        return _take_image(out, n, _libc.free)

    def pick_tile_width(self, batch):
        """Program key the cost model chooses for this graph at this batch size (gwb_graph_pick_tile_width)."""
        key = int(lib().gwb_graph_pick_tile_width(self._h, batch))
        if key == 0:
            raise WitnessCalcError("gwb_graph_pick_tile_width failed")
        return key

    def set_tile_width(self, t):
        if lib().gwb_set_tile_width(self._h, t) != 0:
            raise WitnessCalcError("tile width must be 0 or a power of two in 1..64")

    def inputs_from_json(self, inputs_json):
        """-> uint8 [n_inputs, 32] row (slot 0 = 1); reference src/lib.rs:195-247, 154-181."""
        if isinstance(inputs_json, str):
            inputs_json = inputs_json.encode("utf-8")
        row = np.zeros((self.n_inputs, 32), dtype=np.uint8)
        _call(lib().gwb_inputs_from_json, self._h, inputs_json, row.ctypes.data)
        return row

    def inputs_from_json_batch(self, text):
        """JSON array of input objects or NDJSON -> uint8 [B, n_inputs, 32] (gwb_inputs_from_json_batch)."""
        if isinstance(text, str):
            text = text.encode("utf-8")
        n = ctypes.c_size_t()
        try:  # (the count of input sets: with no room for rows, any text that holds a set is refused for that alone)
            _call(lib().gwb_inputs_from_json_batch, self._h, text, len(text), None, 0, ctypes.byref(n))
        except WitnessCalcError as e:
            if "rows buffer too small" not in str(e):
                raise
        rows = np.zeros((n.value, self.n_inputs, 32), dtype=np.uint8)
        _call(lib().gwb_inputs_from_json_batch, self._h, text, len(text), rows.ctypes.data, n.value, ctypes.byref(n))
        return rows

    def json_to_wtns(self, text, path_pattern, first_index=0, with_status=True):
        """End to end, streaming (gwb_calc_witness_json_to_wtns): JSON array / NDJSON text -> one `.wtns` file per input set
        (path_pattern with one %lu); a set with a non-zero status word gets no file.  Returns (per-set status uint32 [B],
        stats dict); with_status=False passes no status buffer: a failed set then raises."""
        if isinstance(text, str):
            text = text.encode("utf-8")
        n = ctypes.c_size_t()
        cap = max(1, text.count(b"\n") + 1, text.count(b"{"))
        status = np.zeros(cap, dtype=np.uint32)
        es = E2eStats()
        _call(lib().gwb_calc_witness_json_to_wtns, self._h, text, len(text), path_pattern.encode(), first_index, ctypes.byref(n),
              status.ctypes.data if with_status else None, cap if with_status else 0, ctypes.byref(es))
        return status[:n.value], {k: getattr(es, k) for k, _ in E2eStats._fields_}

    def calc_witness_batch(self, inputs, out=None):
        """Host buffers: inputs uint8 [B, n_inputs, 32] -> (witness uint8 [B, W, 32], status uint32 [B]).
        `out`: optional contiguous uint8 [B, W, 32] to fill (e.g. from pinned_rows, which skips the staging copy)."""
        inputs = np.ascontiguousarray(inputs, dtype=np.uint8)
        b = inputs.shape[0]
        assert inputs.shape[1:] == (self.n_inputs, 32), inputs.shape
        if out is None:
            wit = np.empty((b, self.n_witness, 32), dtype=np.uint8)
        else:
            wit = out
            assert wit.dtype == np.uint8 and wit.shape == (b, self.n_witness, 32) and wit.flags["C_CONTIGUOUS"]
        status = np.zeros(b, dtype=np.uint32)
        _call(lib().gwb_calc_witness_batch_host, self._h, inputs.ctypes.data, b, wit.ctypes.data, status.ctypes.data)
        return wit, status

    def calc_witness_batch_device(self, d_inputs, d_witness, d_status, stream=None, montgomery=False, done_event=None):
        """Device-resident: torch uint8 cuda tensors [B, n_inputs, 32] -> [B, W, 32], int32/uint32 [B].
        Asynchronous on `stream` (torch.cuda.Stream) or the current torch stream.  montgomery / done_event
        (torch.cuda.Event, recorded behind the call's last kernel): the prover hand-off of gwb_calc_witness_batch_handoff."""
        import torch
        b = d_inputs.shape[0]
        assert d_inputs.is_cuda and d_witness.is_cuda and d_status.is_cuda
        assert d_inputs.is_contiguous() and d_witness.is_contiguous() and d_status.is_contiguous()
        assert tuple(d_inputs.shape[1:]) == (self.n_inputs, 32) and tuple(d_witness.shape) == (b, self.n_witness, 32)
        s = stream if stream is not None else torch.cuda.current_stream()
        if montgomery or done_event is not None:
            if done_event is not None:
                done_event.record(s)  # (creates the underlying hipEvent_t; the library records it again behind its kernels)
            h = Handoff(ctypes.sizeof(Handoff), _form(montgomery), s.cuda_stream, done_event.cuda_event if done_event is not None else None)
            _call(lib().gwb_calc_witness_batch_handoff, self._h, d_inputs.data_ptr(), b, d_witness.data_ptr(), d_status.data_ptr(), ctypes.byref(h))
        else:
            _call(lib().gwb_calc_witness_batch_device, self._h, d_inputs.data_ptr(), b, d_witness.data_ptr(), d_status.data_ptr(), s.cuda_stream)

    def timing_history(self, max_launches):
        """(interp_ms, pack_ms) float32 arrays of the most recent launches on this handle, oldest first (synchronizes
        on their events); for timing a run of asynchronous calls without a synchronization inside it."""
        a = np.zeros(max_launches, dtype=np.float32)
        b = np.zeros(max_launches, dtype=np.float32)
        n = ctypes.c_size_t(0)
        if lib().gwb_timing_history(self._h, max_launches, a.ctypes.data, b.ctypes.data, ctypes.byref(n)) != 0:
            raise WitnessCalcError("gwb_timing_history failed")
        return a[:n.value], b[:n.value]

    def profile_classes(self, d_inputs, d_witness, d_status):
        """Diagnostic stamped build: {class: (cycles, 0, 0, bundles)} over sampled waves, plus "_sections":
        {"MUL" / "LIN": (top + staged-operand wait, LDS reads + previous bundle's stores, staging issue, arithmetic, ring write, bundles)}."""
        out = np.zeros(96, dtype=np.uint64)
        _call(lib().gwb_profile_classes, self._h, d_inputs.data_ptr(), d_inputs.shape[0], d_witness.data_ptr(), d_status.data_ptr(), out.ctypes.data)
        names = ["INPUT", "MUL", "LIN", "DIV", "CMPZ", "CMPS", "BIT", "IDIVMOD", "TERN", "DIVREQ", "DIVGET", "MULQ"]
        res = {n: tuple(int(x) for x in out[4 * i:4 * i + 4]) for i, n in enumerate(names)}
        res["MULF"] = tuple(int(x) for x in out[64:68])
        res["SCAN"] = tuple(int(x) for x in out[68:72])
        res["_scan_kinds"] = {k: tuple(int(x) for x in out[72 + 4 * i:76 + 4 * i]) for i, k in enumerate(("carry", "division", "convolution", "borrow", "comparison"))}
        res["_sections"] = {"MUL": tuple(int(x) for x in out[48:54]), "LIN": tuple(int(x) for x in out[56:62])}
        # the issue part of section 1 (reads, record refill, previous stores ISSUED; the rest of the section is the wait for the LDS reads)
        res["_issue_part"] = {"MUL": int(out[92]), "LIN": int(out[93])}
        # the divider waves' inline pack (sampled divider waves): cycles spent in pack passes, passes
        res["_pack"] = {"cycles": int(out[94]), "passes": int(out[95])}
        n = int(out[63])
        res["_waves"] = {"n": n, "max_cycles": int(out[54]), "min_cycles": (1 << 40) - int(out[55]) if n else 0,
                         "mean_cycles": int(out[62]) // n if n else 0}
        return res

    def wave_census(self, d_inputs, d_witness, d_status):
        """Diagnostic stamped build (gwb_wave_census): one record per wave of the batch's last interpreter launch that started --
        {"workgroup", "wave" (of the workgroup), "xcc", "se", "sh", "cu", "simd", "divider", "stream", "has_tile", "start", "end"}
        (s_memtime; end 0: the wave had nothing to do).  At most the launch's first 8192 waves."""
        out = np.zeros(3 * 8192, dtype=np.uint64)
        _call(lib().gwb_wave_census, self._h, d_inputs.data_ptr(), d_inputs.shape[0], d_witness.data_ptr(), d_status.data_ptr(), out.ctypes.data, out.size)
        rec = out.reshape(-1, 3)
        idx = [i for i in range(rec.shape[0]) if rec[i, 1]]
        res = []
        for i in idx:
            w0 = int(rec[i, 0])
            role, wpw = (w0 >> 40) & 255, (w0 >> 48) & 255  # (wpw: waves per workgroup)
            res.append({"workgroup": i // wpw, "wave": i % wpw, "xcc": (w0 >> 32) & 15, "se": (w0 >> 13) & 7, "sh": (w0 >> 12) & 1, "cu": (w0 >> 8) & 15, "simd": (w0 >> 4) & 3,
                        "divider": role & 1, "stream": (role >> 1) & 7, "has_tile": (role >> 4) & 1, "start": int(rec[i, 1]), "end": int(rec[i, 2])})
        return res

    def program_stats(self, key=0):
        """Statistics of a compiled program (0: the one the last batch call used): gwb_program_stats."""
        ps = ProgramStats()
        if lib().gwb_program_stats(self._h, key, ctypes.byref(ps)) != 0:
            raise WitnessCalcError("gwb_program_stats: no such program")
        n = ps.n_classes
        return {"tile_width": ps.tile_width, "divider": ps.divider, "streams": ps.streams, "n_bundles": ps.n_bundles,
                "n_fused_nodes": ps.n_fused_nodes, "n_scan_steps": ps.n_scan_steps, "n_conv_products": ps.n_conv_products, "chain_floor_cycles": ps.chain_floor_cycles, "model_wave_cycles": ps.model_wave_cycles, "lanes_active_mean": ps.lanes_active_mean, "values_per_bundle_mean": ps.values_per_bundle_mean,
                "class_bundles": {CLASS_NAMES[c]: int(ps.class_bundles[c]) for c in range(n) if ps.class_bundles[c]},
                "class_nodes": {CLASS_NAMES[c]: int(ps.class_nodes[c]) for c in range(n) if ps.class_nodes[c]}}

    def pack_schedule(self, key):
        """The pack schedule of the program for `key` (gwb_pack_schedule; host only): (pack_order, pack_ready, n_inline)."""
        return _pack_schedule(lambda *a: lib().gwb_pack_schedule(self._h, key, *a))

    def last_timing(self):
        t = Timing()
        if lib().gwb_last_timing(self._h, ctypes.byref(t)) != 0:
            raise WitnessCalcError("gwb_last_timing failed")
        return {n: getattr(t, n) for n, _ in Timing._fields_}


def _pack_schedule(call):
    nw, nr, ni = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    _call(call, None, 0, None, 0, ctypes.byref(nw), ctypes.byref(nr), ctypes.byref(ni))
    order, ready = np.zeros(nw.value, dtype=np.uint32), np.zeros(nr.value, dtype=np.uint32)
    _call(call, order.ctypes.data, order.size, ready.ctypes.data, ready.size, ctypes.byref(nw), ctypes.byref(nr), ctypes.byref(ni))
    return order, ready, int(ni.value)


def pack_schedule_of_blob(blob):
    """The pack schedule a replica derives from an exported program (gwb_pack_schedule_of_blob; host only)."""
    blob = bytes(blob)
    return _pack_schedule(lambda *a: lib().gwb_pack_schedule_of_blob(blob, len(blob), *a))


# -- R1CS satisfaction check (include/graph_witness_r1cs.h, libcwc_r1cs.so built from r1cs/) ------------------------------
R1CS_SATISFIED = 0xFFFFFFFF


def modmul_rate():
    """Measurement aid: Montgomery products per second of the current device (a short probe kernel)."""
    rate = ctypes.c_double()
    if r1cs_lib().gwb_r1cs_modmul_rate(ctypes.byref(rate)) != 0:
        raise WitnessCalcError("gwb_r1cs_modmul_rate failed")
    return rate.value


# -- the Groth16 witness map, shared by R1cs (gwb_r1cs_qap_*) and Groth16 (gwb_zkey_qap_*): `src` is "r1cs" or "zkey" ----------
def _qap_info(h, src):
    info = R1csQapInfo()
    _r1cs_call(getattr(r1cs_lib(), "gwb_%s_qap_info" % src), h, ctypes.byref(info))
    return {n: int(getattr(info, n)) for n, _ in R1csQapInfo._fields_}


def _qap_batch(h, src, witness_rows, montgomery_out):
    if isinstance(witness_rows, tuple):
        witness_rows = witness_rows[0]
    w = np.ascontiguousarray(witness_rows, dtype=np.uint8)
    assert w.ndim == 3 and w.shape[2] == 32, w.shape
    b = w.shape[0]
    out = np.zeros((b, _qap_info(h, src)["domain_size"], 32), dtype=np.uint8)
    _r1cs_call(getattr(r1cs_lib(), "gwb_%s_qap_batch_host" % src), h, w.ctypes.data, w.shape[1], b, out.ctypes.data, _form(montgomery_out))
    return out


def _qap_batch_device(h, src, d_witness, stream, montgomery, montgomery_out):
    import torch
    assert d_witness.is_cuda and d_witness.is_contiguous() and d_witness.dtype == torch.uint8
    assert d_witness.dim() == 3 and d_witness.shape[2] == 32, tuple(d_witness.shape)
    b = d_witness.shape[0]
    n = _qap_info(h, src)["domain_size"]
    out = torch.empty((b, n, 32), dtype=torch.uint8, device=d_witness.device)
    with _device_call(d_witness, stream, (out,)) as s:
        _r1cs_call(getattr(r1cs_lib(), "gwb_%s_qap_batch_device" % src), h, d_witness.data_ptr(), d_witness.shape[1], b, _form(montgomery),
                   out.data_ptr(), _form(montgomery_out), s.cuda_stream)
    return out


class R1cs(_Handle):
    """A circuit's constraint system (`.r1cs` bytes, iden3 binfile v1; BN254, no custom gates) for checking witness rows on the
    GPU: per row, the smallest failing constraint index (R1CS_SATISFIED if none) and the number of failing constraints."""
    _FREE = ("_r1cs_lib", "gwb_r1cs_free")

    def __init__(self, data):
        self._h = ctypes.c_void_p()
        data = bytes(data)
        _r1cs_call(r1cs_lib().gwb_r1cs_load, data, len(data), ctypes.byref(self._h))
        info = R1csInfo()
        r1cs_lib().gwb_r1cs_info(self._h, ctypes.byref(info))
        self.info = {n: int(getattr(info, n)) for n, _ in R1csInfo._fields_}

    def set_tile_width(self, t):
        """Witness rows per wavefront of the check kernel: a power of two in 1..64, or 0 = from the batch size."""
        if r1cs_lib().gwb_r1cs_set_tile_width(self._h, t) != 0:
            raise WitnessCalcError("tile width must be 0 or a power of two in 1..64")

    def check_batch(self, witness_rows):
        """Host rows uint8 [B, W, 32] (canonical), or the (witness, status) pair of Graph.calc_witness_batch ->
        (first_failed uint32 [B], n_failed uint32 [B]).  Synchronous."""
        if isinstance(witness_rows, tuple):
            witness_rows = witness_rows[0]
        w = np.ascontiguousarray(witness_rows, dtype=np.uint8)
        assert w.ndim == 3 and w.shape[2] == 32, w.shape
        b = w.shape[0]
        first = np.zeros(b, dtype=np.uint32)
        nfail = np.zeros(b, dtype=np.uint32)
        _r1cs_call(r1cs_lib().gwb_r1cs_check_batch_host, self._h, w.ctypes.data, w.shape[1], b, first.ctypes.data, nfail.ctypes.data)
        return first, nfail

    def check_batch_device(self, d_witness, stream=None, montgomery=False):
        """Device rows (torch uint8 cuda tensor [B, W, 32], canonical or Montgomery form) -> (first_failed, n_failed) as int32
        cuda tensors [B] (first_failed -1 = R1CS_SATISFIED).  Asynchronous on `stream` (torch.cuda.Stream) or the current
        torch stream: put it behind Graph.calc_witness_batch_device on the same stream."""
        import torch
        assert d_witness.is_cuda and d_witness.is_contiguous() and d_witness.dtype == torch.uint8
        assert d_witness.dim() == 3 and d_witness.shape[2] == 32, tuple(d_witness.shape)
        b = d_witness.shape[0]
        first = torch.empty(b, dtype=torch.int32, device=d_witness.device)
        nfail = torch.empty(b, dtype=torch.int32, device=d_witness.device)
        with _device_call(d_witness, stream) as s:
            _r1cs_call(r1cs_lib().gwb_r1cs_check_batch_device, self._h, d_witness.data_ptr(), d_witness.shape[1], b, _form(montgomery),
                       first.data_ptr(), nfail.data_ptr(), s.cuda_stream)
        return first, nfail

    def check_wtns(self, wtns):
        """One `.wtns` image -> (first_failed, n_failed); first_failed is R1CS_SATISFIED when every constraint holds."""
        wtns = bytes(wtns)
        first, nfail = ctypes.c_uint32(), ctypes.c_uint32()
        _r1cs_call(r1cs_lib().gwb_r1cs_check_wtns, self._h, wtns, len(wtns), ctypes.byref(first), ctypes.byref(nfail))
        return int(first.value), int(nfail.value)

    # -- Groth16 witness map (h, the scalars of the prover's H-point MSM; definition in include/graph_witness_r1cs.h) --------
    def qap_info(self):
        """{n_rows, domain_power, domain_size, workspace_bytes_per_row} of the QAP domain; raises for a domain above 2^27."""
        return _qap_info(self._h, "r1cs")

    def qap_batch(self, witness_rows, montgomery_out=False):
        """Host rows uint8 [B, W, 32] (canonical), or the (witness, status) pair of Graph.calc_witness_batch -> h as uint8
        [B, n, 32] (canonical, or Montgomery with montgomery_out).  Synchronous."""
        return _qap_batch(self._h, "r1cs", witness_rows, montgomery_out)

    def qap_batch_device(self, d_witness, stream=None, montgomery=False, montgomery_out=False):
        """Device rows (torch uint8 cuda tensor [B, W, 32], canonical or Montgomery form) -> h as a uint8 cuda tensor [B, n, 32].
        Asynchronous on `stream` (torch.cuda.Stream) or the current torch stream: put it behind
        Graph.calc_witness_batch_device on the same stream."""
        return _qap_batch_device(self._h, "r1cs", d_witness, stream, montgomery, montgomery_out)

    def qap_time_phases(self, on=True):
        """Measurement aid: record HIP events around the phases of later QAP calls (see qap_phase_ms)."""
        if r1cs_lib().gwb_r1cs_qap_time_phases(self._h, 1 if on else 0) != 0:
            raise WitnessCalcError("gwb_r1cs_qap_time_phases failed")

    def qap_phase_ms(self):
        """Waits for the last QAP call -> {evaluation, inverse_outer, fused_inner, forward_outer} in ms (its last sub-batch)."""
        return _phase_ms(r1cs_lib().gwb_r1cs_qap_phase_ms, ("evaluation", "inverse_outer", "fused_inner", "forward_outer"),
                         "no QAP phase times (qap_time_phases not on, or no QAP call yet)", self._h)

    def qap_wtns(self, wtns, montgomery_out=False):
        """One `.wtns` image -> h as uint8 [n, 32]."""
        wtns = bytes(wtns)
        h = np.zeros((self.qap_info()["domain_size"], 32), dtype=np.uint8)
        _r1cs_call(r1cs_lib().gwb_r1cs_qap_wtns, self._h, wtns, len(wtns), h.ctypes.data, _form(montgomery_out))
        return h


# -- Groth16 prover (include/graph_witness_groth16.h, libcwc_r1cs.so) ----------------------------------------------------------
GROTH16_PROOF_BYTES = 256
GROTH16_PHASES = ("witness_map", "scalars_sort", "g1_msms", "g2_msm", "assembly")


def _rs_array(rs, b):
    """None, or r / s pairs (ints below r) / uint8 [B, 2, 32] -> a contiguous uint8 array or None"""
    if rs is None:
        return None
    if isinstance(rs, np.ndarray):
        a = np.ascontiguousarray(rs, dtype=np.uint8)
    else:
        a = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for pair in rs for x in pair), dtype=np.uint8).copy()
    assert a.size == b * 64, "rs must hold [batch][2][32 B]"
    return a


def _dec(b):
    return str(int.from_bytes(bytes(b), "little"))


def proof_json(proof):
    """256 proof bytes -> snarkjs's proof.json dict (decimal strings; z = "1", or "0" for the point at infinity)"""
    p = bytes(proof)
    c = [_dec(p[32 * k:32 * k + 32]) for k in range(8)]
    z = lambda lo, hi: "1" if any(p[lo:hi]) else "0"  # noqa: E731
    return {"pi_a": [c[0], c[1], z(0, 64)], "pi_b": [[c[2], c[3]], [c[4], c[5]], [z(64, 192), "0"]],
            "pi_c": [c[6], c[7], z(192, 256)], "protocol": "groth16", "curve": "bn128"}


class Groth16(_Handle):
    """A circuit's Groth16 proving key (`.zkey` bytes, snarkjs's Groth16 format): proofs of witness rows on the GPU, 256 bytes
    per row (A.x, A.y, B.x.c0, B.x.c1, B.y.c0, B.y.c1, C.x, C.y, canonical little-endian).  The witness map comes from the
    key's own section 4 (what snarkjs and rapidsnark do), or, when an R1cs of the same circuit is given, from that.  Section 4
    is turned into the prover's arrays at the first call that needs it; what that step refuses (a value >= r, no coefficients,
    a domain the transform cannot take) is raised there, not here.  check_g2=True also runs check_g2() on the loaded key (on
    the GPU); by default the key's G2 points are checked for the curve equation alone, as before."""
    _FREE = ("_r1cs_lib", "gwb_zkey_free")

    def __init__(self, zkey_bytes, r1cs=None, check_g2=False):
        self._h = ctypes.c_void_p()
        self.r1cs = r1cs
        data = bytes(zkey_bytes)
        _r1cs_call(r1cs_lib().gwb_zkey_load, data, len(data), ctypes.byref(self._h))
        info = ZkeyInfo()
        r1cs_lib().gwb_zkey_info(self._h, ctypes.byref(info))
        self.info = {n: int(getattr(info, n)) for n, _ in ZkeyInfo._fields_}
        if check_g2:
            self.check_g2()

    def _r1cs_handle(self):
        return None if self.r1cs is None else self.r1cs._h

    def check_r1cs(self, r1cs=None):
        """Raises unless the key belongs to `r1cs` (default: the handle's own): section 4, summed per (matrix, constraint, signal),
        equals the A and B combinations of the R1cs plus the nPublic + 1 public rows, and the size fields agree.  The message
        names the smallest differing (constraint, matrix, signal).  Host only.  A zkey holds no C matrix, so the C sides are
        not compared."""
        r1cs = self.r1cs if r1cs is None else r1cs
        if r1cs is None:
            raise WitnessCalcError("check_r1cs: no R1cs given and the handle has none")
        _r1cs_call(r1cs_lib().gwb_zkey_check_r1cs, self._h, r1cs._h)

    def check_g2(self):
        """Raises unless beta2, gamma2, delta2 and every B2 point (section 7) lie in G2's order-r subgroup; checked on the
        current GPU (synchronous).  The message names the first offender: "zkey: beta2 is not in the order-r subgroup of G2", or
        "zkey: section 7 (B2) point 12 is not in the order-r subgroup of G2 (3 of 70 points are not)".  A proof made with a
        B2 point outside the subgroup is refused by every verifier (VERIFY_SUBGROUP)."""
        _r1cs_call(r1cs_lib().gwb_zkey_check_g2, self._h)

    # -- the witness map of section 4 on its own (always from the zkey, whether or not the handle has an R1cs) -----------------
    def set_tile_width(self, t):
        """Witness rows per wavefront of the section-4 evaluation kernel: a power of two in 1..64, or 0 = from the batch size."""
        if r1cs_lib().gwb_zkey_set_tile_width(self._h, t) != 0:
            raise WitnessCalcError("tile width must be 0 or a power of two in 1..64")

    def qap_info(self):
        """{n_rows, domain_power, domain_size, workspace_bytes_per_row}; n_rows = 1 + the largest constraint index in section 4."""
        return _qap_info(self._h, "zkey")

    def qap_batch(self, witness_rows, montgomery_out=False):
        """Host rows uint8 [B, nVars, 32] (canonical) -> h as uint8 [B, n, 32] (canonical, or Montgomery with montgomery_out), as
        R1cs.qap_batch.  Synchronous."""
        return _qap_batch(self._h, "zkey", witness_rows, montgomery_out)

    def qap_batch_device(self, d_witness, stream=None, montgomery=False, montgomery_out=False):
        """Device rows (torch uint8 cuda tensor [B, nVars, 32], canonical or Montgomery form) -> h as a uint8 cuda tensor
        [B, n, 32], as R1cs.qap_batch_device.  Asynchronous on `stream` or the current torch stream."""
        return _qap_batch_device(self._h, "zkey", d_witness, stream, montgomery, montgomery_out)

    def prove_batch(self, rows, rs=None):
        """Host rows uint8 [B, nVars, 32] (canonical), or the (witness, status) pair of Graph.calc_witness_batch -> uint8
        [B, 256].  rs: [B] pairs (r, s) of ints below r, or uint8 [B, 2, 32]; None draws them from getrandom().  Synchronous."""
        if isinstance(rows, tuple):
            rows = rows[0]
        w = np.ascontiguousarray(rows, dtype=np.uint8)
        assert w.ndim == 3 and w.shape[2] == 32, w.shape
        b = w.shape[0]
        rsa = _rs_array(rs, b)
        out = np.zeros((b, GROTH16_PROOF_BYTES), dtype=np.uint8)
        _r1cs_call(r1cs_lib().gwb_groth16_prove_batch_host, self._h, self._r1cs_handle(), w.ctypes.data, w.shape[1], b,
                   None if rsa is None else rsa.ctypes.data, out.ctypes.data)
        return out

    def prove_batch_device(self, d_w, stream=None, montgomery=False, rs=None):
        """Device rows (torch uint8 cuda tensor [B, nVars, 32], canonical or Montgomery form) -> a uint8 cuda tensor [B, 256].
        Asynchronous on `stream` or the current torch stream (rs is read before the call returns)."""
        import torch
        assert d_w.is_cuda and d_w.is_contiguous() and d_w.dtype == torch.uint8
        assert d_w.dim() == 3 and d_w.shape[2] == 32, tuple(d_w.shape)
        b = d_w.shape[0]
        rsa = _rs_array(rs, b)
        out = torch.empty((b, GROTH16_PROOF_BYTES), dtype=torch.uint8, device=d_w.device)
        with _device_call(d_w, stream, (out,)) as s:
            _r1cs_call(r1cs_lib().gwb_groth16_prove_batch_device, self._h, self._r1cs_handle(), d_w.data_ptr(), d_w.shape[1], b, _form(montgomery),
                       None if rsa is None else rsa.ctypes.data, out.data_ptr(), s.cuda_stream)
        return out

    def prove_batch_compressed_device(self, d_w, stream=None, montgomery=False, rs=None):
        """prove_batch_device, then groth16_compress_proofs_device on the same stream -> a uint8 cuda tensor [B, 128] (arkworks'
        compressed form: include/graph_witness_groth16_compressed.h).  The 256-byte proofs stay on the device."""
        s = _stream_of(d_w, stream)
        return groth16_compress_proofs_device(self.prove_batch_device(d_w, stream=s, montgomery=montgomery, rs=rs), stream=s)

    def prove_batch_compressed(self, rows, rs=None):
        """Host rows as prove_batch takes them -> uint8 [B, 128], proved and compressed on the GPU.  Synchronous."""
        import torch
        if isinstance(rows, tuple):
            rows = rows[0]
        w = np.array(rows, dtype=np.uint8)
        assert w.ndim == 3 and w.shape[2] == 32, w.shape
        return self.prove_batch_compressed_device(torch.from_numpy(w).cuda(), rs=rs).cpu().numpy()

    def prove_wtns(self, wtns, rs=None):
        """One `.wtns` image -> (proof dict, public signals) in snarkjs's proof.json / public.json shape."""
        wtns = bytes(wtns)
        rsa = _rs_array(rs, 1)
        out = np.zeros(GROTH16_PROOF_BYTES, dtype=np.uint8)
        _r1cs_call(r1cs_lib().gwb_groth16_prove_wtns, self._h, self._r1cs_handle(), wtns, len(wtns), None if rsa is None else rsa.ctypes.data,
                   out.ctypes.data)
        # the values section of the (validated) image: wire i at 32 i
        n_sec = int.from_bytes(wtns[8:12], "little")
        off, values = 12, None
        for _ in range(n_sec):
            t, size = int.from_bytes(wtns[off:off + 4], "little"), int.from_bytes(wtns[off + 4:off + 12], "little")
            if t == 2:
                values = wtns[off + 12:off + 12 + size]
            off += 12 + size
        public = [_dec(values[32 * i:32 * i + 32]) for i in range(1, self.info["n_public"] + 1)]
        return proof_json(out), public

    @classmethod
    def setup(cls, r1cs, trapdoor=None):
        """A proving key made for `r1cs` by groth16_setup (single party: see its trust statement), loaded against it."""
        return cls(groth16_setup(r1cs, trapdoor), r1cs)

    @classmethod
    def setup_ptau(cls, r1cs, ptau, delta=None, lagrange="auto", check_g2=False):
        """A proving key made for `r1cs` from a powers-of-tau file by groth16_setup_ptau (see its trust statement), loaded
        against it.  check_g2: as groth16_setup_ptau's."""
        return cls(groth16_setup_ptau(r1cs, ptau, delta, lagrange, check_g2=check_g2), r1cs)

    def verifying_key(self):
        """The zkey's verifying key (Groth16VerifyingKey)."""
        return Groth16VerifyingKey._from_zkey_handle(self._h)

    def time_phases(self, on=True):
        """Measurement aid: record HIP events around the phases of later prove calls (see phase_ms)."""
        if r1cs_lib().gwb_groth16_time_phases(self._h, 1 if on else 0) != 0:
            raise WitnessCalcError("gwb_groth16_time_phases failed")

    def phase_ms(self):
        """Waits for the last prove call -> {witness_map, scalars_sort, g1_msms, g2_msm, assembly} in ms (its last sub-batch)."""
        return _phase_ms(r1cs_lib().gwb_groth16_phase_ms, GROTH16_PHASES, "no prover phase times (time_phases not on, or no prove call yet)", self._h)


# -- Groth16 key setup (include/graph_witness_groth16_setup.h, libcwc_r1cs.so) ------------------------------------------------
GROTH16_SETUP_PHASES = ("lagrange", "column_sums", "key_scalars", "g1_muls", "g2_muls_affine")


def groth16_setup(r1cs, trapdoor=None):
    """The Groth16 proving key of an R1cs as `.zkey` bytes, made on the GPU (circuit-specific setup; synchronous).  trapdoor:
    (tau, alpha, beta, gamma, delta), ints in [1, r) with tau^2n != 1, or None: drawn and discarded.  Single party: whoever
    knows the trapdoor can forge proofs, so this is for development, tests and deployments where the key's maker is trusted
    with all five values (groth16_setup_ptau takes tau, alpha and beta from a public ceremony instead).  Section 10 of the file has no circuit hash and no contributions."""
    vals = None
    if trapdoor is not None:
        vals = [int(x) for x in trapdoor]
        if len(vals) != 5:
            raise WitnessCalcError("trapdoor: 5 values expected (tau, alpha, beta, gamma, delta), %d given" % len(vals))
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    with _secret_scalars(vals, ["trapdoor: %s is not in [0, 2^256)" % name for name in ("tau", "alpha", "beta", "gamma", "delta")]) as buf:
        _r1cs_call(r1cs_lib().gwb_groth16_setup, r1cs._h, buf, ctypes.byref(out), ctypes.byref(n))
    return _take_image(out, n)


def bn254_gen_mul_batch_device(d_scalars, group, stream=None):
    """Measurement and test aid: device scalars (uint8 cuda [n, 32], canonical little-endian; values >= r are reduced) -> k_i
    times the generator of G1 (group 1: uint8 cuda [n, 64]) or G2 (group 2: [n, 128]), canonical affine coordinates, zero bytes
    for the point at infinity.  Asynchronous on `stream` or the current stream."""
    import torch
    n = d_scalars.shape[0]
    assert tuple(d_scalars.shape) == (n, 32) and d_scalars.is_cuda and d_scalars.is_contiguous() and d_scalars.dtype == torch.uint8
    if group not in (1, 2):
        raise WitnessCalcError("group must be 1 or 2")
    out = torch.empty((n, 64 * group), dtype=torch.uint8, device=d_scalars.device)
    with _device_call(d_scalars, stream, (out,)) as s:
        _r1cs_call(r1cs_lib().gwb_bn254_gen_mul_batch_device, d_scalars.data_ptr(), n, group, out.data_ptr(), s.cuda_stream)
    return out


def groth16_setup_phase_ms():
    """{lagrange, column_sums, key_scalars, g1_muls, g2_muls_affine} in ms of the process's last groth16_setup call."""
    return _phase_ms(r1cs_lib().gwb_groth16_setup_phase_ms, GROTH16_SETUP_PHASES, "no setup phase times (no groth16_setup call yet)")


# -- Groth16 key setup from a powers-of-tau file (include/graph_witness_groth16_ptau.h, libcwc_r1cs.so) -------------------------
GROTH16_SETUP_PTAU_PHASES = ("point_check", "idft_g1", "idft_g2", "column_sums_g1", "column_sums_g2", "delta_scale", "affine")
PTAU_LAGRANGE_MODES = {"auto": 0, "file": 1, "compute": 2}


def _ptau_buffer(ptau):
    """(object that keeps the memory alive, address, length) of bytes, a bytearray, an mmap or a numpy array, without a copy
    where the object allows it.  The caller holds the first in a local for as long as the address is in use."""
    if isinstance(ptau, bytes):
        return ptau, ctypes.cast(ctypes.c_char_p(ptau), ctypes.c_void_p), len(ptau)
    arr = np.frombuffer(ptau, dtype=np.uint8)
    return arr, ctypes.c_void_p(arr.ctypes.data), arr.size


def _lagrange_mode(lagrange):
    if lagrange not in PTAU_LAGRANGE_MODES:
        raise WitnessCalcError("lagrange must be one of %s" % ", ".join(PTAU_LAGRANGE_MODES))
    return PTAU_LAGRANGE_MODES[lagrange]


def ptau_info(ptau):
    """{power, ceremony_power, prepared, n_contributions} of a `.ptau` image (bytes or any buffer, an mmap included).  Host
    only: header and section table, no device."""
    keep, addr, n = _ptau_buffer(ptau)
    info = PtauInfo()
    _r1cs_call(r1cs_lib().gwb_ptau_info, addr, n, ctypes.byref(info))
    return {"power": int(info.power), "ceremony_power": int(info.ceremony_power), "prepared": bool(info.prepared),
            "n_contributions": int(info.n_contributions)}


def ptau_check(ptau, domain_power, lagrange="auto"):
    """Host only: raises WitnessCalcError with the message groth16_setup_ptau would give for this file and a circuit of domain
    2^domain_power (the points it would read are checked on the host)."""
    keep, addr, n = _ptau_buffer(ptau)
    _r1cs_call(r1cs_lib().gwb_ptau_check, addr, n, int(domain_power), _lagrange_mode(lagrange))


def ptau_check_g2(ptau, domain_power, lagrange="auto"):
    """Raises WitnessCalcError unless the G2 points that groth16_setup_ptau reads from this file for a circuit of domain
    2^domain_power lie in G2's order-r subgroup: betaG2 and tauG2[0 .. n) when the Lagrange forms are computed, tauG2[0] and level
    domain_power of section 13 when they are read.  The header, the plan and alpha1, beta1, beta2 are checked first, on the host,
    with ptau_check's messages; the points are then checked on the current GPU in bounded pieces (synchronous).  The message
    names section and index: "ptau: section 3 (tauG2) point 5 is not in the order-r subgroup of G2"."""
    keep, addr, n = _ptau_buffer(ptau)
    _r1cs_call(r1cs_lib().gwb_ptau_check_g2, addr, n, int(domain_power), _lagrange_mode(lagrange))


def groth16_setup_ptau(r1cs, ptau, delta=None, lagrange="auto", check_g2=False):
    """The Groth16 proving key of an R1cs as `.zkey` bytes, made on the GPU from a powers-of-tau file (what snarkjs
    `groth16 setup` does; synchronous).  tau, alpha and beta are the ceremony's; gamma = 1.  delta: an int in [1, r), or None:
    drawn, applied and discarded, after which soundness rests on the ceremony behind the file and on this call's runner
    having discarded delta (a single-party phase 2; knowing delta alone is enough to forge).  delta = 1 is the state of
    snarkjs `zkey new`: a key to hand to a phase-2 ceremony, not to use.  lagrange: "auto" reads the file's prepared sections
    when it has them, "file" requires them, "compute" ignores them.  check_g2=True first runs ptau_check_g2 for the circuit's
    domain: without it the file's G2 points are checked for the curve equation alone, and a point outside the order-r subgroup
    ends up in a key whose proofs every verifier refuses."""
    mode = _lagrange_mode(lagrange)
    if check_g2:
        ptau_check_g2(ptau, r1cs.qap_info()["domain_power"], lagrange)
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    with _secret_scalars(None if delta is None else [int(delta)], ["delta is not in [0, 2^256)"]) as buf:
        keep, addr, n_in = _ptau_buffer(ptau)
        _r1cs_call(r1cs_lib().gwb_groth16_setup_ptau, r1cs._h, addr, n_in, buf, mode, ctypes.byref(out), ctypes.byref(n))
    return _take_image(out, n)


def bn254_point_idft_batch_device(d_points, group, stream=None):
    """Measurement and test aid: device points (uint8 cuda [2^m, 64] for group 1, [2^m, 128] for group 2; canonical affine
    coordinates, zero bytes for infinity; 1 <= m <= 27) -> their inverse DFT over the group, (1 / N) sum_i w_N^(-k i) P_i, in
    natural order and the same form.  Asynchronous on `stream` or the current stream."""
    import torch
    if group not in (1, 2):
        raise WitnessCalcError("group must be 1 or 2")
    n = d_points.shape[0]
    assert tuple(d_points.shape) == (n, 64 * group) and d_points.is_cuda and d_points.is_contiguous() and d_points.dtype == torch.uint8
    log_n = n.bit_length() - 1
    if n < 2 or n != 1 << log_n:
        raise WitnessCalcError("the number of points must be a power of two, 2 at the least")
    out = torch.empty_like(d_points)
    with _device_call(d_points, stream, (d_points, out)) as s:
        _r1cs_call(r1cs_lib().gwb_bn254_point_idft_batch_device, d_points.data_ptr(), log_n, group, out.data_ptr(), s.cuda_stream)
    return out


def groth16_setup_ptau_phase_ms():
    """{point_check, idft_g1, idft_g2, column_sums_g1, column_sums_g2, delta_scale, affine} in ms of the process's last
    groth16_setup_ptau call."""
    return _phase_ms(r1cs_lib().gwb_groth16_setup_ptau_phase_ms, GROTH16_SETUP_PTAU_PHASES, "no setup phase times (no groth16_setup_ptau call yet)")


# -- Groth16 phase-2 contributions (include/graph_witness_groth16_contribute.h, libcwc_r1cs.so) ---------------------------------
GROTH16_CONTRIBUTE_PHASES = ("load", "scale", "affine")
CONTRIBUTION_HASH_BYTES = 64


def groth16_contribute(zkey, name="", delta=None):
    """One phase-2 contribution to a Groth16 key on the GPU (synchronous): `.zkey` bytes -> (new `.zkey` bytes, the 64-byte
    contribution hash to publish).  delta1 and delta2 are multiplied by the secret, sections 8 (C) and 9 (H) by its inverse, a
    record with a proof of knowledge is appended to section 10, everything else stays byte for byte.  delta: an int in
    [1, r) for reproducible keys, or None: drawn, applied and discarded.  name: at most 255 bytes of UTF-8.  The records are
    this library's own (BLAKE2b transcript, its own challenge derivation): `snarkjs zkey verify` does not accept them, while
    sections 1 to 9 are ordinary and every Groth16 prover and verifier works with the key."""
    nm = _name_bytes(name)
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    digest = ctypes.create_string_buffer(CONTRIBUTION_HASH_BYTES)
    with _secret_scalars(None if delta is None else [int(delta)], ["delta is not in [0, 2^256)"]) as buf:
        data = bytes(zkey)
        _r1cs_call(r1cs_lib().gwb_groth16_contribute, data, len(data), nm, buf, ctypes.byref(out), ctypes.byref(n), digest)
    return _take_image(out, n), digest.raw


def groth16_contribute_phase_ms():
    """{load, scale, affine} in ms of the process's last groth16_contribute call, summed over its pieces."""
    return _phase_ms(r1cs_lib().gwb_groth16_contribute_phase_ms, GROTH16_CONTRIBUTE_PHASES, "no contribution phase times (no groth16_contribute call yet)")


# -- the random beacon of both phases (include/graph_witness_groth16_beacon.h) ---------------------------------------------------
def _beacon_call(call, addr, n_in, beacon_hash, iterations_exp, name):
    nm = _name_bytes(name)
    digest_in = bytes(beacon_hash)
    e = int(iterations_exp)
    if not 0 <= e < (1 << 32):
        raise WitnessCalcError("beacon: numIterationsExp %d is not in [10, 63]" % e)
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    digest = ctypes.create_string_buffer(CONTRIBUTION_HASH_BYTES)
    _r1cs_call(call, addr, n_in, nm, digest_in, len(digest_in), e, ctypes.byref(out), ctypes.byref(n), digest)
    return _take_image(out, n), digest.raw


def groth16_beacon(zkey, beacon_hash, iterations_exp, name=""):
    """The random beacon that closes phase 2 (snarkjs `zkey beacon`; synchronous, on the GPU): `.zkey` bytes -> (new `.zkey`
    bytes, the 64-byte hash of the new record).  It is the contribution of groth16_contribute whose secret and nonce nobody
    chooses: both are derived from beacon_hash (bytes, 1 to 255 of them: a value that did not exist when the last participant
    contributed) by 2^iterations_exp chained SHA-256 on the host, 10 <= iterations_exp <= min(63, CWC_BEACON_MAX_EXP, default
    28).  The record has type 1 and carries both parameters, so anybody can recompute it, and the verifications do; two runs
    give identical bytes.  The derivation is this library's own: snarkjs does not accept the record."""
    data = bytes(zkey)
    return _beacon_call(r1cs_lib().gwb_groth16_beacon, data, len(data), beacon_hash, iterations_exp, name)


def ptau_beacon(ptau, beacon_hash, iterations_exp, name=""):
    """The random beacon that closes phase 1 (snarkjs `powersoftau beacon`; synchronous, on the GPU): a `.ptau` image -> (new
    `.ptau` bytes, the new record's nextChallenge).  The contribution of ptau_contribute with tau', alpha', beta' and the three
    nonces derived from beacon_hash and iterations_exp as for groth16_beacon; prepared sections are dropped as there."""
    keep, addr, n_in = _ptau_buffer(ptau)
    return _beacon_call(r1cs_lib().gwb_ptau_beacon, addr, n_in, beacon_hash, iterations_exp, name)


def beacon_scalars(phase, beacon_hash, iterations_exp):
    """Host only, for audit: the scalars a beacon derives, as ints in [1, r): phase 1 -> [tau', alpha', beta', s_0, s_1, s_2],
    phase 2 -> [delta', s].  They are public."""
    digest_in = bytes(beacon_hash)
    count = {1: 6, 2: 2}.get(phase)
    e = int(iterations_exp)
    out = ctypes.create_string_buffer(32 * 6)
    if count is None or not 0 <= e < (1 << 32) or r1cs_lib().gwb_beacon_scalars(phase, digest_in, len(digest_in), e, out) != 0:
        raise WitnessCalcError("beacon: phase 1 or 2, a beaconHash of 1 to 255 bytes and numIterationsExp in [10, 63] and at most "
                               "CWC_BEACON_MAX_EXP expected")
    return [int.from_bytes(out.raw[32 * j:32 * j + 32], "little") for j in range(count)]


def sha256(data):
    """SHA-256 by the library's host code, the link of the beacon's hash chain (an aid beside gwb_blake2b512)."""
    data = bytes(data)
    out = ctypes.create_string_buffer(32)
    r1cs_lib().gwb_sha256(data, len(data), out)
    return out.raw


def _beacon_items(call, addr, n_in, k, typ):
    """(iterations_exp, beacon_hash) of record k from its raw parameters (items 02 and 03; the last of each), each None when
    the record has no such item; (None, None) for a record of type 0."""
    if typ != 1:
        return None, None
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    _r1cs_call(call, addr, n_in, k, ctypes.byref(out), ctypes.byref(n))
    par = _take_image(out, n)
    exp, digest, i = None, None, 0
    while i < len(par):  # the section's reader has checked the items' lengths
        tag = par[i]
        if tag == 2:
            exp = par[i + 1]
            i += 2
        else:
            if tag == 3:
                digest = par[i + 2:i + 2 + par[i + 1]]
            i += 2 + par[i + 1]
    return exp, digest


def _require_beacon(records, what):
    if not records or records[-1]["type"] != 1:
        raise WitnessCalcError("%s: the last contribution is not a beacon" % what)


def zkey_contributions(zkey):
    """Section 10 of a `.zkey` (host only): {"cs_hash", "contributions": [{"name", "type", "delta_after", "g1_s", "g1_sx",
    "g2_spx", "transcript", "hash", "iterations_exp", "beacon_hash"}]}.  Points are canonical little-endian bytes (64 for G1,
    128 for G2: x.c0, x.c1, y.c0, y.c1), type is 0 (contribution) or 1 (beacon), hash is what the participant published,
    iterations_exp and beacon_hash are a beacon's parameters (None for type 0).  Nothing is verified beyond the section's
    form; a malformed section raises with a message starting "zkey: section 10"."""
    data = bytes(zkey)
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    _r1cs_call(r1cs_lib().gwb_zkey_contributions, data, len(data), ctypes.byref(out), ctypes.byref(n))
    img = _take_image(out, n)
    count = int.from_bytes(img[64:68], "little")
    off, recs = 68, []
    for k in range(count):
        fixed = img[off:off + 448]
        typ, name_len = (int.from_bytes(img[off + 448 + 4 * i:off + 452 + 4 * i], "little") for i in range(2))
        off += 456
        recs.append({"name": img[off:off + name_len].decode("utf-8", "replace"), "type": typ, "delta_after": fixed[:64], "g1_s": fixed[64:128],
                     "g1_sx": fixed[128:192], "g2_spx": fixed[192:320], "transcript": fixed[320:384], "hash": fixed[384:448]})
        recs[-1]["iterations_exp"], recs[-1]["beacon_hash"] = _beacon_items(r1cs_lib().gwb_zkey_contribution_params, data, len(data), k, typ)
        off += name_len
    return {"cs_hash": img[:64], "contributions": recs}


def groth16_verify_contributions(zkey, require_beacon=False):
    """Checks every contribution record of a key on the GPU and returns their hashes, oldest first ([] for a key without
    records, whose delta must then be the generator).  Raises WitnessCalcError naming the first failing record and rule, for
    example "zkey: contribution 2: deltaAfter is not deltaPrev times the proven secret".  This checks the chain of deltas; it does not compare the key with its circuit or
    its powers-of-tau file: groth16_verify_key does.  A beacon record's key must be the one its parameters derive.
    require_beacon=True additionally raises "zkey: the last contribution is not a beacon" for an accepted key that does not
    end on one."""
    data = bytes(zkey)
    records = zkey_contributions(data)["contributions"]
    room = len(records)
    hashes = ctypes.create_string_buffer(max(1, room * CONTRIBUTION_HASH_BYTES))
    n = ctypes.c_size_t(room)
    _r1cs_call(r1cs_lib().gwb_zkey_verify_contributions, data, len(data), hashes, ctypes.byref(n))
    if require_beacon:
        _require_beacon(records, "zkey")
    return [hashes.raw[64 * k:64 * k + 64] for k in range(n.value)]


def groth16_verify_contribution_step(prev, next, seed=None):
    """Checks on the GPU that the key `next` is the key `prev` after exactly one contribution: the new record, the delta
    points, the untouched sections byte for byte, and sections 8 and 9 through random linear combinations of their points
    (a wrong point passes with probability about 2^-128 over the seed).  seed: 32 bytes for a reproducible check, or None to
    draw them.  Raises WitnessCalcError naming what differs."""
    a, b = bytes(prev), bytes(next)
    _r1cs_call(r1cs_lib().gwb_zkey_verify_step, a, len(a), b, len(b), _seed32(seed))


def bn254_g1_scale_batch_device(d_points, k, stream=None):
    """Measurement and test aid of the contribution's kernel: device G1 points (uint8 cuda [n, 64], canonical affine, zero
    bytes for infinity, not validated) -> k times each, the same form, for one int k in [0, 2^256).  Asynchronous on `stream`
    or the current stream."""
    import torch
    n = d_points.shape[0]
    assert tuple(d_points.shape) == (n, 64) and d_points.is_cuda and d_points.is_contiguous() and d_points.dtype == torch.uint8
    out = torch.empty_like(d_points)
    with _device_call(d_points, stream, (d_points, out)) as s:
        _r1cs_call(r1cs_lib().gwb_bn254_g1_scale_batch_device, d_points.data_ptr(), n, int(k).to_bytes(32, "little"), out.data_ptr(), s.cuda_stream)
    return out


def _lincomb128_device(group, d_points, d_rho, stream):
    import torch
    n, width = d_points.shape[0], 64 * group
    assert tuple(d_points.shape) == (n, width) and d_points.is_cuda and d_points.is_contiguous() and d_points.dtype == torch.uint8
    assert tuple(d_rho.shape) == (n, 16) and d_rho.is_cuda and d_rho.is_contiguous() and d_rho.dtype == torch.uint8
    out = torch.empty((width,), dtype=torch.uint8, device=d_points.device)
    call = r1cs_lib().gwb_bn254_g1_lincomb128_device if group == 1 else r1cs_lib().gwb_bn254_g2_lincomb128_device
    with _device_call(d_points, stream, (d_points, d_rho, out)) as s:
        _r1cs_call(call, d_points.data_ptr(), d_rho.data_ptr(), n, out.data_ptr(), s.cuda_stream)
    return out


def bn254_g1_lincomb128_device(d_points, d_rho, stream=None):
    """Measurement and test aid of the step check's kernels: device G1 points (uint8 cuda [n, 64], canonical affine) and
    128-bit little-endian scalars (uint8 cuda [n, 16]) -> sum_i rho_i P_i as uint8 cuda [64].  Asynchronous on `stream` or the
    current stream."""
    return _lincomb128_device(1, d_points, d_rho, stream)


def bn254_g2_lincomb128_device(d_points, d_rho, stream=None):
    """The same in G2, the aid of the powers check's kernels: device G2 points (uint8 cuda [n, 128], canonical affine x.c0,
    x.c1, y.c0, y.c1, zero bytes for infinity) and 128-bit scalars (uint8 cuda [n, 16]) -> sum_i rho_i P_i as uint8 cuda [128]."""
    return _lincomb128_device(2, d_points, d_rho, stream)


def _seed32(seed):
    if seed is None:
        return None
    seed = bytes(seed)
    if len(seed) != 32:
        raise WitnessCalcError("seed: 32 bytes expected")
    return seed


def ptau_check_powers(ptau, domain_power, seed=None):
    """Raises WitnessCalcError unless the monomial points that groth16_setup_ptau reads from this file for a circuit of domain
    n = 2^domain_power under lagrange="compute" are what their sections say: tauG1[0 .. 2n) and tauG2[0 .. n) consecutive powers
    of one tau, alphaTauG1[0 .. n) and betaTauG1[0 .. n) those powers times their first point, betaG2 with the same beta.  First
    ptau_check's refusals and ptau_check_g2's subgroup rule, with their messages; then random linear combinations of the points
    on the current GPU and five pairing equations (synchronous; a wrong point passes with probability about 2^-128 over the
    seed).  seed: 32 bytes for a reproducible check, or None to draw them.  The message names the section: "ptau: section 2
    (tauG1): the first 2n points are not consecutive powers of the tau of section 3".  Not checked: points beyond the
    prefixes (ptau_verify checks the whole file), the prepared sections 12 to 15, records made by snarkjs."""
    seed = _seed32(seed)
    keep, addr, n = _ptau_buffer(ptau)
    _r1cs_call(r1cs_lib().gwb_ptau_check_powers, addr, n, int(domain_power), seed)


# -- the prepared sections 12 to 15 of a `.ptau` (include/graph_witness_groth16_ptau.h) ------------------------------------------
PTAU_PREPARE_PHASES = ("load", "idft_g1", "idft_g2", "affine")
PTAU_ALL_LEVELS = 0xffffffff


def ptau_prepare_phase2(ptau):
    """What snarkjs `powersoftau prepare phase2` does, on the GPU (synchronous): a `.ptau` image (bytes or any buffer, an mmap
    included) -> the image with its Lagrange sections 12 to 15 made from the monomial sections 2 to 5, as bytes.  Every other
    section is carried byte for byte in the input's order; sections 12 to 15 follow, replacing any the input had.  Level m of
    a Lagrange section is Lag_m of the first 2^m monomial points at point offset 2^m - 1; section 12's extra level power + 1
    takes the point at infinity for the input that section 2 lacks.  groth16_setup_ptau and groth16_verify_key read the
    result under lagrange="file" and skip their own transforms.  The file is parsed and sized before the GPU is touched; all
    levels of one section must fit CWC_GROTH16_WORKSPACE_MB on the device.  No snarkjs-prepared file was compared."""
    keep, addr, n_in = _ptau_buffer(ptau)
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    _r1cs_call(r1cs_lib().gwb_ptau_prepare_phase2, addr, n_in, ctypes.byref(out), ctypes.byref(n))
    return _take_image(out, n)


def ptau_prepare_phase_ms():
    """{load, idft_g1, idft_g2, affine} in ms of the process's last ptau_prepare_phase2 call, summed over the four sections."""
    return _phase_ms(r1cs_lib().gwb_ptau_prepare_phase_ms, PTAU_PREPARE_PHASES, "no prepare phase times (no ptau_prepare_phase2 call yet)")


def ptau_check_lagrange(ptau, domain_power=None, seed=None):
    """Raises WitnessCalcError unless the Lagrange sections 12 to 15 of a prepared `.ptau` are the Lagrange forms of its
    monomial sections 2 to 5.  domain_power=p: the levels groth16_setup_ptau reads for a circuit of domain 2^p under
    lagrange="file" (level p of the four sections, level p + 1 of section 12); None: every level of every section.  First
    ptau_check's refusals, point faults among the points read and the refusal of a file without prepared sections, with
    their messages; for section 13 the subgroup rule of ptau_check_g2; then per section one random linear combination of
    the Lagrange points against one of the monomial points on the current GPU, compared as points (synchronous; a wrong point
    passes with probability about 2^-128 over the seed).  seed: 32 bytes for a reproducible check, or None to draw them.  The
    message names the section and the level: "ptau: section 14 (lagrange alphaTauG1) level 3 does not hold the Lagrange
    forms of section 4".  Not checked: that sections 2 to 5 are powers of one tau (ptau_check_powers)."""
    seed = _seed32(seed)
    keep, addr, n = _ptau_buffer(ptau)
    _r1cs_call(r1cs_lib().gwb_ptau_check_lagrange, addr, n, PTAU_ALL_LEVELS if domain_power is None else int(domain_power), seed)


def _lincomb_device(group, d_points, d_scalars, form, stream):
    import torch
    if form not in ("canonical", "montgomery"):
        raise WitnessCalcError("form must be canonical or montgomery")
    n, width = d_points.shape[0], 64 * group
    assert tuple(d_points.shape) == (n, width) and d_points.is_cuda and d_points.is_contiguous() and d_points.dtype == torch.uint8
    assert tuple(d_scalars.shape) == (n, 32) and d_scalars.is_cuda and d_scalars.is_contiguous() and d_scalars.dtype == torch.uint8
    out = torch.empty((width,), dtype=torch.uint8, device=d_points.device)
    call = r1cs_lib().gwb_bn254_g1_lincomb_device if group == 1 else r1cs_lib().gwb_bn254_g2_lincomb_device
    with _device_call(d_points, stream, (d_points, d_scalars, out)) as s:
        _r1cs_call(call, d_points.data_ptr(), d_scalars.data_ptr(), n, 0 if form == "canonical" else 1, out.data_ptr(), s.cuda_stream)
    return out


def bn254_g1_lincomb_device(d_points, d_scalars, form="canonical", stream=None):
    """Measurement and test aid of the Lagrange check's right-hand side, beside bn254_g1_lincomb128_device: device G1 points
    (uint8 cuda [n, 64], affine in `form`, "canonical" or "montgomery"; zero bytes for infinity) and canonical little-endian
    scalars below r (uint8 cuda [n, 32]) -> sum_i scalar_i P_i as uint8 cuda [64] in the same form.  Asynchronous on `stream`
    or the current stream."""
    return _lincomb_device(1, d_points, d_scalars, form, stream)


def bn254_g2_lincomb_device(d_points, d_scalars, form="canonical", stream=None):
    """The same in G2: uint8 cuda [n, 128] points (x.c0, x.c1, y.c0, y.c1) and [n, 32] scalars -> uint8 cuda [128]."""
    return _lincomb_device(2, d_points, d_scalars, form, stream)


# -- the powers-of-tau ceremony itself (include/graph_witness_groth16_ceremony.h) ---------------------------------------------------
PTAU_CONTRIBUTE_PHASES = ("load", "scalars", "mul_g1", "mul_g2", "affine")
PTAU_VERIFY_SKIP_RECORDS = 1
MUL_METHODS = {"window": 0, "plain": 1}


def ptau_new(power):
    """What snarkjs `powersoftau new` does (host only): the `.ptau` bytes of a new ceremony of the given power, 1 to 28, with
    tau = alpha = beta = 1: every point is its group's generator and section 7 holds no record.  Such a file is the start of a
    ceremony, nothing more: keys made from it before anyone contributed can be forged against by everybody."""
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    _r1cs_call(r1cs_lib().gwb_ptau_new, int(power), ctypes.byref(out), ctypes.byref(n))
    return _take_image(out, n)


def ptau_contribute(ptau, name="", secrets=None):
    """One contribution to a powers-of-tau ceremony on the GPU (synchronous): a `.ptau` image (bytes or any buffer, an mmap
    included) -> (new `.ptau` bytes, the 64-byte hash to publish: the new record's nextChallenge).  Every point of sections 2
    to 5 is multiplied by its own scalar (tau'^i, alpha' tau'^i, beta' tau'^i), betaG2 by beta', and a record with three proofs
    of knowledge is appended to section 7; section 1 and unknown sections stay byte for byte; the prepared sections 12 to 15 are
    dropped (ptau_prepare_phase2 makes them again).  secrets: (tau', alpha', beta') as ints in [1, r) for reproducible files, or
    None: drawn, applied and discarded.  name: at most 255 bytes of UTF-8.  The records are this library's own: `snarkjs
    powersoftau verify` does not accept them, while sections 1 to 6 are ordinary."""
    nm = _name_bytes(name)
    refusal = "secrets: three integers in [0, 2^256) expected (tau, alpha, beta)"
    xs = None
    if secrets is not None:
        xs = [int(x) for x in secrets]
        if len(xs) != 3:
            raise WitnessCalcError(refusal)
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    digest = ctypes.create_string_buffer(CONTRIBUTION_HASH_BYTES)
    with _secret_scalars(xs, [refusal] * 3) as buf:
        keep, addr, n_in = _ptau_buffer(ptau)
        _r1cs_call(r1cs_lib().gwb_ptau_contribute, addr, n_in, nm, buf, ctypes.byref(out), ctypes.byref(n), digest)
    return _take_image(out, n), digest.raw


def ptau_contribute_phase_ms():
    """{load, scalars, mul_g1, mul_g2, affine} in ms of the process's last ptau_contribute call, summed over its pieces."""
    return _phase_ms(r1cs_lib().gwb_ptau_contribute_phase_ms, PTAU_CONTRIBUTE_PHASES, "no contribution phase times (no ptau_contribute call yet)")


PTAU_RECORD_POINTS = (("tau_g1", 64), ("tau_g2", 128), ("alpha_g1", 64), ("beta_g1", 64), ("beta_g2", 128), ("tau_g1_s", 64), ("tau_g1_sx", 64),
                      ("alpha_g1_s", 64), ("alpha_g1_sx", 64), ("beta_g1_s", 64), ("beta_g1_sx", 64), ("tau_g2_spx", 128), ("alpha_g2_spx", 128),
                      ("beta_g2_spx", 128))


def ptau_contributions(ptau):
    """Section 7 of a `.ptau` (host only): [{"name", "type", the five after-values "tau_g1", "tau_g2", "alpha_g1", "beta_g1",
    "beta_g2", the nine key points "tau_g1_s", "tau_g1_sx", ..., "beta_g2_spx", "next_challenge"}], oldest first.  Points are
    canonical little-endian bytes (64 for G1, 128 for G2: x.c0, x.c1, y.c0, y.c1), type is 0 (contribution) or 1 (beacon),
    next_challenge is the hash the participant published; "iterations_exp" and "beacon_hash" are a beacon's parameters (None
    for type 0).  Nothing is verified beyond the section's form; a malformed section raises with a message starting "ptau:
    section 7"."""
    keep, addr, n_in = _ptau_buffer(ptau)
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    _r1cs_call(r1cs_lib().gwb_ptau_contributions, addr, n_in, ctypes.byref(out), ctypes.byref(n))
    img = _take_image(out, n)
    count = int.from_bytes(img[:4], "little")
    off, recs = 4, []
    for k in range(count):
        rec = {}
        for key, size in PTAU_RECORD_POINTS:
            rec[key] = img[off:off + size]
            off += size
        rec["next_challenge"] = img[off:off + 64]
        rec["type"], name_len = (int.from_bytes(img[off + 64 + 4 * i:off + 68 + 4 * i], "little") for i in range(2))
        off += 72
        rec["name"] = img[off:off + name_len].decode("utf-8", "replace")
        off += name_len
        rec["iterations_exp"], rec["beacon_hash"] = _beacon_items(r1cs_lib().gwb_ptau_contribution_params, addr, n_in, k, rec["type"])
        recs.append(rec)
    return recs


def ptau_verify(ptau, records=True, seed=None, require_beacon=False):
    """Verifies a ceremony file on the GPU (synchronous) and returns the hashes of its records, oldest first.  Every record is
    checked against the one before it (its challenge, its three proofs of knowledge, its after-values; the first against the
    generators), the last record's after-values against the file's points, and then the whole file: every tauG2 in the order-r
    subgroup, every section consecutive powers of one tau through random linear combinations of ALL its points and five
    pairing equations (a wrong point passes with probability about 2^-128 over the seed).  records=False passes over section 7:
    for files that carry snarkjs's records, which this library cannot verify.  seed: 32 bytes for a reproducible check, or None
    to draw them.  Raises WitnessCalcError naming the first failing record and rule, or the section, for example "ptau:
    contribution 2: alphaG1 is not the previous alphaG1 times the proven secret".  A beacon record's keys must be the ones
    its parameters derive.  require_beacon=True additionally raises "ptau: the last contribution is not a beacon" for an accepted
    file that does not end on one."""
    seed = _seed32(seed)
    keep, addr, n_in = _ptau_buffer(ptau)
    room = ptau_info(ptau)["n_contributions"]
    hashes = ctypes.create_string_buffer(max(1, room * CONTRIBUTION_HASH_BYTES))
    n = ctypes.c_size_t(room)
    _r1cs_call(r1cs_lib().gwb_ptau_verify, addr, n_in, 0 if records else PTAU_VERIFY_SKIP_RECORDS, seed, hashes, ctypes.byref(n))
    if require_beacon:
        _require_beacon(ptau_contributions(ptau), "ptau")
    return [hashes.raw[64 * k:64 * k + 64] for k in range(min(room, n.value))]


def ptau_verify_step(prev, next, seed=None):
    """Checks on the GPU that the file `next` is the file `prev` after exactly one contribution: section 1 identical, one record
    more with the earlier ones byte for byte, the new record's proofs against the five anchor points of `prev` (tauG1[1],
    tauG2[1], alphaTauG1[0], betaTauG1[0], betaG2), its after-values in `next`, and the whole-file check of ptau_verify on
    `next`.  Works on top of records this library cannot verify.  Raises WitnessCalcError naming what fails."""
    seed = _seed32(seed)
    ka, aa, na = _ptau_buffer(prev)
    kb, ab, nb = _ptau_buffer(next)
    _r1cs_call(r1cs_lib().gwb_ptau_verify_step, aa, na, ab, nb, seed)


def _mul_batch_device(group, d_points, d_scalars, form, method, stream):
    import torch
    if form not in ("canonical", "montgomery"):
        raise WitnessCalcError("form must be canonical or montgomery")
    if method not in MUL_METHODS:
        raise WitnessCalcError("method must be one of %s" % ", ".join(MUL_METHODS))
    n, width = d_points.shape[0], 64 * group
    assert tuple(d_points.shape) == (n, width) and d_points.is_cuda and d_points.is_contiguous() and d_points.dtype == torch.uint8
    assert tuple(d_scalars.shape) == (n, 32) and d_scalars.is_cuda and d_scalars.is_contiguous() and d_scalars.dtype == torch.uint8
    out = torch.empty_like(d_points)
    call = r1cs_lib().gwb_bn254_g1_mul_batch_device if group == 1 else r1cs_lib().gwb_bn254_g2_mul_batch_device
    with _device_call(d_points, stream, (d_points, d_scalars, out)) as s:
        _r1cs_call(call, d_points.data_ptr(), d_scalars.data_ptr(), n, 0 if form == "canonical" else 1, MUL_METHODS[method], out.data_ptr(), s.cuda_stream)
    return out


def bn254_g1_mul_batch_device(d_points, d_scalars, form="canonical", method="window", stream=None):
    """Measurement and test aid of the ceremony's multiplication kernel: device G1 points (uint8 cuda [n, 64], affine in `form`,
    "canonical" or "montgomery"; zero bytes for infinity, not validated) and canonical little-endian scalars below r (uint8 cuda
    [n, 32]) -> scalar_i P_i for every i, uint8 cuda [n, 64] in the same form.  method: "window" (signed digits, the table of
    multiples in LDS) or "plain" (double-and-add per thread).  Asynchronous on `stream` or the current stream."""
    return _mul_batch_device(1, d_points, d_scalars, form, method, stream)


def bn254_g2_mul_batch_device(d_points, d_scalars, form="canonical", method="window", stream=None):
    """The same in G2: uint8 cuda [n, 128] points (x.c0, x.c1, y.c0, y.c1) and [n, 32] scalars -> uint8 cuda [n, 128]."""
    return _mul_batch_device(2, d_points, d_scalars, form, method, stream)


GROTH16_VERIFY_KEY_PHASES = ("remake", "lincomb", "pairings")
VERIFY_KEY_SKIP_RECORDS, VERIFY_KEY_CHECK_PTAU = 1, 2


def groth16_verify_key(zkey, r1cs, ptau, lagrange="compute", records=True, check_ptau=False, seed=None, check_lagrange=False, require_beacon=False):
    """Checks on the GPU that `zkey` is the honest key of the R1cs and the powers-of-tau file (bytes or any buffer, an mmap
    included), with a delta that only its recorded contributions touched (what `snarkjs zkey verify` answers; synchronous),
    and returns the contribution hashes, oldest first.  The key is remade from circuit and file with delta = 1; section 4 is
    compared with the circuit, sections 1, 3, 5, 6, 7 and the header's alpha1, beta1, beta2, gamma2 with the remade key byte
    for byte, the records by groth16_verify_contributions's rules with the csHash of the remade key, and sections 8 (C) and 9
    (H) against the remade key's and delta2 through random linear combinations (a wrong point passes with probability about
    2^-128 over the seed).  Raises WitnessCalcError with the first rule that fails, for example "zkey verify: section 8 (C) is
    not the remade key's section divided by delta".  lagrange: "compute" (default) keeps the verdict off the file's prepared
    sections 12 to 15; "auto" and "file" read them, verified only under check_lagrange.  records=False passes over section 10
    (for keys that carry snarkjs's records, which this library cannot verify): the points are still checked against circuit,
    file and the key's own delta.  check_ptau=True first runs ptau_check_powers for the circuit's domain.  check_lagrange=True, with
    lagrange "auto" or "file", first runs ptau_check_lagrange for the circuit's domain (under "auto" only when the file has
    prepared sections), and its failure is the verdict: the prepared sections that the remake reads are then verified against
    the monomial ones, for much less than "compute" spends on making them again; with "compute" the flag has nothing to
    check.  Not verified: records made by snarkjs in the file, and its points beyond the prefixes a setup reads (ptau_verify
    checks this library's records and the whole file).  require_beacon=True additionally raises "zkey: the last contribution is
    not a beacon" for an accepted key that does not end on one."""
    mode = _lagrange_mode(lagrange)
    seed = _seed32(seed)
    data = bytes(zkey)
    key_records = zkey_contributions(data)["contributions"]
    room = len(key_records)
    if check_lagrange and lagrange != "compute" and (lagrange == "file" or ptau_info(ptau)["prepared"]):
        ptau_check_lagrange(ptau, r1cs.qap_info()["domain_power"], seed)
    hashes = ctypes.create_string_buffer(max(1, room * CONTRIBUTION_HASH_BYTES))
    n = ctypes.c_size_t(room)
    flags = (0 if records else VERIFY_KEY_SKIP_RECORDS) | (VERIFY_KEY_CHECK_PTAU if check_ptau else 0)
    keep, addr, n_in = _ptau_buffer(ptau)
    _r1cs_call(r1cs_lib().gwb_zkey_verify_key, data, len(data), r1cs._h, addr, n_in, mode, flags, seed, hashes, ctypes.byref(n))
    if require_beacon:
        _require_beacon(key_records, "zkey")
    return [hashes.raw[64 * k:64 * k + 64] for k in range(n.value)]


def groth16_verify_key_phase_ms():
    """{remake, lincomb, pairings} in ms of the process's last accepted groth16_verify_key call (host clock)."""
    return _phase_ms(r1cs_lib().gwb_zkey_verify_key_phase_ms, GROTH16_VERIFY_KEY_PHASES, "no key check phase times (no accepted groth16_verify_key call yet)")


# -- Groth16 verifier (include/graph_witness_groth16_verify.h, libcwc_r1cs.so) ------------------------------------------------
GT_BYTES = 384
VERIFY_VALID, VERIFY_PUBLIC, VERIFY_POINT, VERIFY_SUBGROUP, VERIFY_EQUATION = 0, 1, 2, 3, 4
VERIFY_STATUS_NAMES = {0: "VALID", 1: "PUBLIC", 2: "POINT", 3: "SUBGROUP", 4: "EQUATION"}


def _json_g1(b):
    """64 canonical bytes -> snarkjs [x, y, z] (z "0" and x = y = "0" for infinity)"""
    if not any(b):
        return ["0", "1", "0"]
    return [_dec(b[:32]), _dec(b[32:64]), "1"]


def _json_g2(b):
    if not any(b):
        return [["0", "0"], ["1", "0"], ["0", "0"]]
    return [[_dec(b[:32]), _dec(b[32:64])], [_dec(b[64:96]), _dec(b[96:128])], ["1", "0"]]


def _int32(x, what):
    v = int(x)
    if not 0 <= v < (1 << 256):
        raise WitnessCalcError("%s: %d is not in [0, 2^256)" % (what, v))
    return v.to_bytes(32, "little")


def _from_json_g1(p, what):
    if not isinstance(p, (list, tuple)) or len(p) != 3:
        raise WitnessCalcError("%s: a G1 point is [x, y, z]" % what)
    if str(p[2]) == "0":
        return bytes(64)
    if str(p[2]) != "1":
        raise WitnessCalcError("%s: z must be \"1\" (affine) or \"0\" (infinity)" % what)
    return _int32(p[0], what) + _int32(p[1], what)


def _from_json_g2(p, what):
    if not isinstance(p, (list, tuple)) or len(p) != 3 or any(not isinstance(c, (list, tuple)) or len(c) != 2 for c in p):
        raise WitnessCalcError("%s: a G2 point is [[x0, x1], [y0, y1], [z0, z1]]" % what)
    z = [str(c) for c in p[2]]
    if z == ["0", "0"]:
        return bytes(128)
    if z != ["1", "0"]:
        raise WitnessCalcError("%s: z must be [\"1\", \"0\"] (affine) or [\"0\", \"0\"] (infinity)" % what)
    return b"".join(_int32(c, what) for c in (p[0][0], p[0][1], p[1][0], p[1][1]))


def _gt_json(b):
    """384 GT bytes -> snarkjs's vk_alphabeta_12 nesting [[[c0.b0.a0, c0.b0.a1], ...], [...]]"""
    v = [_dec(b[32 * k:32 * k + 32]) for k in range(12)]
    return [[[v[6 * i + 2 * j], v[6 * i + 2 * j + 1]] for j in range(3)] for i in range(2)]


def _public_array(publics, b, n):
    """[B] lists of ints / uint8 [B, n, 32] -> contiguous uint8 [B, n, 32]; ints must lie in [0, 2^256)"""
    if isinstance(publics, np.ndarray):
        a = np.ascontiguousarray(publics, dtype=np.uint8).reshape(b, n, 32)
    else:
        publics = list(publics)
        assert len(publics) == b, "one list of public signals per proof"
        a = np.zeros((b, n, 32), dtype=np.uint8)
        for i, row in enumerate(publics):
            row = list(row)
            if len(row) != n:
                raise WitnessCalcError("%d public signals in row %d, the key has nPublic %d" % (len(row), i, n))
            for k, x in enumerate(row):
                a[i, k] = np.frombuffer(_int32(x, "public signal"), dtype=np.uint8)
    return a


class Groth16VerifyingKey(_Handle):
    """A Groth16 verifying key (nPublic, alpha1, beta2, gamma2, delta2, IC) for checking proofs on the GPU: one status per proof
    (VERIFY_VALID, VERIFY_PUBLIC, VERIFY_POINT, VERIFY_SUBGROUP, VERIFY_EQUATION; include/graph_witness_groth16_verify.h)."""
    _FREE = ("_r1cs_lib", "gwb_g16vk_free")

    def __init__(self, points, n_public):
        """points: canonical bytes alpha1 (64), beta2, gamma2, delta2 (128 each), IC (64 each)"""
        points = bytes(points)
        self._h = ctypes.c_void_p()
        _r1cs_call(r1cs_lib().gwb_g16vk_load, points, len(points), int(n_public), ctypes.byref(self._h))
        self.n_public = int(n_public)

    @classmethod
    def _from_zkey_handle(cls, zh):
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        _r1cs_call(r1cs_lib().gwb_g16vk_from_zkey, zh, ctypes.byref(self._h))
        n = ctypes.c_uint32()
        r1cs_lib().gwb_g16vk_info(self._h, ctypes.byref(n))
        self.n_public = int(n.value)
        return self

    @classmethod
    def from_zkey(cls, zkey_bytes):
        """The verifying key of a `.zkey` (bytes)."""
        zh = ctypes.c_void_p()
        data = bytes(zkey_bytes)
        _r1cs_call(r1cs_lib().gwb_zkey_load, data, len(data), ctypes.byref(zh))
        try:
            return cls._from_zkey_handle(zh)
        finally:
            r1cs_lib().gwb_zkey_free(zh)

    @classmethod
    def from_json(cls, vk):
        """snarkjs's verification_key.json (dict); vk_alphabeta_12 is ignored, as snarkjs ignores it."""
        if not isinstance(vk, dict):
            raise WitnessCalcError("verification key: not a JSON object")
        for k in ("protocol", "nPublic", "vk_alpha_1", "vk_beta_2", "vk_gamma_2", "vk_delta_2", "IC"):
            if k not in vk:
                raise WitnessCalcError("verification key: no \"%s\"" % k)
        if vk["protocol"] != "groth16":
            raise WitnessCalcError("verification key: protocol is not \"groth16\"")
        pts = _from_json_g1(vk["vk_alpha_1"], "vk_alpha_1")
        for k in ("vk_beta_2", "vk_gamma_2", "vk_delta_2"):
            pts += _from_json_g2(vk[k], k)
        pts += b"".join(_from_json_g1(p, "IC[%d]" % i) for i, p in enumerate(vk["IC"]))
        return cls(pts, int(vk["nPublic"]))

    def points(self):
        """canonical bytes alpha1, beta2, gamma2, delta2, IC (the constructor's layout)"""
        out = ctypes.create_string_buffer(448 + 64 * (self.n_public + 1))
        if r1cs_lib().gwb_g16vk_points(self._h, out, len(out)) != 0:
            raise WitnessCalcError("gwb_g16vk_points failed")
        return out.raw

    def alphabeta(self):
        """e(alpha1, beta2) as GT_BYTES bytes (computed on the GPU at the first call)"""
        out = ctypes.create_string_buffer(GT_BYTES)
        _r1cs_call(r1cs_lib().gwb_g16vk_alphabeta, self._h, out)
        return out.raw

    def to_json(self):
        """snarkjs's verification_key.json shape (vk_alphabeta_12 from the GPU)"""
        p = self.points()
        return {"protocol": "groth16", "curve": "bn128", "nPublic": self.n_public, "vk_alpha_1": _json_g1(p[:64]),
                "vk_beta_2": _json_g2(p[64:192]), "vk_gamma_2": _json_g2(p[192:320]), "vk_delta_2": _json_g2(p[320:448]),
                "vk_alphabeta_12": _gt_json(self.alphabeta()),
                "IC": [_json_g1(p[448 + 64 * i:512 + 64 * i]) for i in range(self.n_public + 1)]}

    def verify_batch(self, proofs, publics):
        """Host proofs uint8 [B, 256] and public signals ([B] lists of ints, or uint8 [B, nPublic, 32]) -> uint32 status [B].
        Synchronous."""
        p = np.ascontiguousarray(proofs, dtype=np.uint8).reshape(-1, GROTH16_PROOF_BYTES)
        b = p.shape[0]
        s = _public_array(publics, b, self.n_public)
        out = np.zeros(b, dtype=np.uint32)
        _r1cs_call(r1cs_lib().gwb_groth16_verify_batch_host, self._h, p.ctypes.data, s.ctypes.data, self.n_public, b, out.ctypes.data)
        return out

    def verify_batch_device(self, d_proofs, d_public, stream=None):
        """Device proofs (torch uint8 cuda [B, 256]) and signals (uint8 cuda [B, nPublic, 32], canonical) -> an int32 cuda
        tensor [B] of statuses.  Asynchronous on `stream` or the current torch stream."""
        import torch
        assert d_proofs.is_cuda and d_proofs.is_contiguous() and d_proofs.dtype == torch.uint8 and d_proofs.dim() == 2
        assert d_proofs.shape[1] == GROTH16_PROOF_BYTES, tuple(d_proofs.shape)
        b = d_proofs.shape[0]
        assert d_public.is_cuda and d_public.is_contiguous() and d_public.dtype == torch.uint8
        assert tuple(d_public.shape) == (b, self.n_public, 32), tuple(d_public.shape)
        out = torch.empty(b, dtype=torch.int32, device=d_proofs.device)
        with _device_call(d_proofs, stream, (out,)) as s:
            _r1cs_call(r1cs_lib().gwb_groth16_verify_batch_device, self._h, d_proofs.data_ptr(), d_public.data_ptr() if self.n_public else None,
                       self.n_public, b, out.data_ptr(), s.cuda_stream)
        return out

    @classmethod
    def from_compressed(cls, data):
        """A key from arkworks' compressed bytes (232 + 32 (nPublic + 1); include/graph_witness_groth16_compressed.h), decoded
        strictly on the host.  Refusals start "verifying key:" and name the point."""
        data = bytes(data)
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        _r1cs_call(r1cs_lib().gwb_g16vk_load_compressed, data, len(data), ctypes.byref(self._h))
        n = ctypes.c_uint32()
        r1cs_lib().gwb_g16vk_info(self._h, ctypes.byref(n))
        self.n_public = int(n.value)
        return self

    def to_compressed(self):
        """the key's compressed bytes (from_compressed's layout)"""
        out = ctypes.create_string_buffer(232 + 32 * (self.n_public + 1))
        if r1cs_lib().gwb_g16vk_compressed(self._h, out, len(out)) != 0:
            raise WitnessCalcError("gwb_g16vk_compressed failed")
        return out.raw

    def verify_batch_compressed(self, cproofs, publics):
        """verify_batch on compressed proofs, uint8 [B, 128]: decoded on the GPU, then verified; a refused encoding gives
        VERIFY_POINT (behind VERIFY_PUBLIC, as the rule order has it).  Synchronous."""
        p = np.ascontiguousarray(cproofs, dtype=np.uint8).reshape(-1, GROTH16_CPROOF_BYTES)
        b = p.shape[0]
        s = _public_array(publics, b, self.n_public)
        out = np.zeros(b, dtype=np.uint32)
        _r1cs_call(r1cs_lib().gwb_groth16_verify_batch_compressed_host, self._h, p.ctypes.data, s.ctypes.data, self.n_public, b, out.ctypes.data)
        return out

    def verify_batch_compressed_device(self, d_cproofs, d_public, stream=None):
        """verify_batch_device on compressed device proofs (torch uint8 cuda [B, 128]) -> an int32 cuda tensor [B] of statuses.
        Asynchronous on `stream` or the current torch stream."""
        import torch
        assert d_cproofs.is_cuda and d_cproofs.is_contiguous() and d_cproofs.dtype == torch.uint8 and d_cproofs.dim() == 2
        assert d_cproofs.shape[1] == GROTH16_CPROOF_BYTES, tuple(d_cproofs.shape)
        b = d_cproofs.shape[0]
        assert d_public.is_cuda and d_public.is_contiguous() and d_public.dtype == torch.uint8
        assert tuple(d_public.shape) == (b, self.n_public, 32), tuple(d_public.shape)
        out = torch.empty(b, dtype=torch.int32, device=d_cproofs.device)
        with _device_call(d_cproofs, stream, (d_cproofs, out)) as s:
            _r1cs_call(r1cs_lib().gwb_groth16_verify_batch_compressed_device, self._h, d_cproofs.data_ptr(), d_public.data_ptr() if self.n_public else None,
                       self.n_public, b, out.data_ptr(), s.cuda_stream)
        return out

    def verify(self, proof, public):
        """snarkjs proof.json (dict) and public.json (list of decimal strings) -> True when VERIFY_VALID."""
        pb = _from_json_g1(proof["pi_a"], "pi_a") + _from_json_g2(proof["pi_b"], "pi_b") + _from_json_g1(proof["pi_c"], "pi_c")
        return int(self.verify_batch(np.frombuffer(pb, dtype=np.uint8).reshape(1, -1), [[int(x) for x in public]])[0]) == VERIFY_VALID


def bn254_pairing_batch_device(d_g1, d_g2, stream=None):
    """Measurement and test aid: device G1 points (uint8 cuda [n, 64]) and G2 points ([n, 128]), canonical, in their groups
    (not validated) -> e(P_i, Q_i) as a uint8 cuda tensor [n, GT_BYTES].  Asynchronous on `stream` or the current stream."""
    import torch
    n = d_g1.shape[0]
    assert tuple(d_g1.shape) == (n, 64) and tuple(d_g2.shape) == (n, 128)
    assert d_g1.is_cuda and d_g2.is_cuda and d_g1.is_contiguous() and d_g2.is_contiguous()
    out = torch.empty((n, GT_BYTES), dtype=torch.uint8, device=d_g1.device)
    with _device_call(d_g1, stream, (out,)) as s:
        _r1cs_call(r1cs_lib().gwb_bn254_pairing_batch_device, d_g1.data_ptr(), d_g2.data_ptr(), n, out.data_ptr(), s.cuda_stream)
    return out


G2_CHECK_METHODS = {"fast": 0, "order": 1}


def bn254_g2_check_batch_device(d_points, montgomery=False, method="fast", stream=None):
    """Measurement and test aid, and the kernel behind Groth16.check_g2 and ptau_check_g2: device G2 points (uint8 cuda [n, 128]:
    x.c0, x.c1, y.c0, y.c1, canonical little-endian or, with montgomery, as the files store them; zero bytes = infinity) -> a
    uint32 cuda tensor [n]: VERIFY_VALID (in the order-r subgroup, infinity included), VERIFY_POINT (a coordinate >= q, or not on
    the twist) or VERIFY_SUBGROUP (on the twist, outside the subgroup).  method "fast" is the psi criterion
    [x + 1] P + psi([x] P) + psi^2([x] P) = psi^3([2x] P), "order" is [r] P = O.  Asynchronous on `stream` or the current stream."""
    import torch
    if method not in G2_CHECK_METHODS:
        raise WitnessCalcError("method must be one of %s" % ", ".join(G2_CHECK_METHODS))
    n = d_points.shape[0]
    assert tuple(d_points.shape) == (n, 128) and d_points.is_cuda and d_points.is_contiguous() and d_points.dtype == torch.uint8
    out = torch.empty(n, dtype=torch.uint32, device=d_points.device)
    with _device_call(d_points, stream, (d_points, out)) as s:
        _r1cs_call(r1cs_lib().gwb_bn254_g2_check_batch_device, d_points.data_ptr() if n else None, n, _form(montgomery), G2_CHECK_METHODS[method],
                   out.data_ptr() if n else None, s.cuda_stream)
    return out


# -- compressed points, proofs and keys (include/graph_witness_groth16_compressed.h, libcwc_r1cs.so) ------------------------------
GROTH16_CPROOF_BYTES = 128


def _codec_args(d_in, width):
    import torch
    assert d_in.is_cuda and d_in.is_contiguous() and d_in.dtype == torch.uint8 and d_in.dim() == 2 and d_in.shape[1] == width, tuple(d_in.shape)
    return d_in.shape[0]


def _compress_batch_device(group, d_points, montgomery, stream):
    import torch
    n = _codec_args(d_points, 64 * group)
    out = torch.empty((n, 32 * group), dtype=torch.uint8, device=d_points.device)
    with _device_call(d_points, stream, (d_points, out)) as s:
        _r1cs_call(r1cs_lib().gwb_bn254_compress_batch_device, d_points.data_ptr() if n else None, n, group, _form(montgomery),
                   out.data_ptr() if n else None, s.cuda_stream)
    return out


def _decompress_batch_device(group, d_in, montgomery, stream):
    import torch
    n = _codec_args(d_in, 32 * group)
    out = torch.empty((n, 64 * group), dtype=torch.uint8, device=d_in.device)
    status = torch.empty(n, dtype=torch.int32, device=d_in.device)
    with _device_call(d_in, stream, (d_in, out, status)) as s:
        _r1cs_call(r1cs_lib().gwb_bn254_decompress_batch_device, d_in.data_ptr() if n else None, n, group, _form(montgomery),
                   out.data_ptr() if n else None, status.data_ptr() if n else None, s.cuda_stream)
    return out, status


def bn254_g1_compress_batch_device(d_points, montgomery=False, stream=None):
    """Device G1 points (uint8 cuda [n, 64]: x, y, canonical little-endian or, with montgomery, as the files store them; zero bytes
    = infinity; not validated) -> their compressed form, a uint8 cuda tensor [n, 32] (arkworks' CanonicalSerialize, Compress::Yes:
    include/graph_witness_groth16_compressed.h).  Asynchronous on `stream` or the current torch stream."""
    return _compress_batch_device(1, d_points, montgomery, stream)


def bn254_g2_compress_batch_device(d_points, montgomery=False, stream=None):
    """The same for G2 points: uint8 cuda [n, 128] (x.c0, x.c1, y.c0, y.c1) -> [n, 64]."""
    return _compress_batch_device(2, d_points, montgomery, stream)


def bn254_g1_decompress_batch_device(d_in, montgomery=False, stream=None):
    """Compressed device G1 points (uint8 cuda [n, 32]) -> (points, status): a uint8 cuda tensor [n, 64] in the asked form and an int32
    cuda tensor [n], VERIFY_VALID or, beside the point (0, 0), VERIFY_POINT for an encoding that strict decoding refuses (both
    flags, the infinity flag beside a nonzero bit, x >= q, no root).  Asynchronous on `stream` or the current torch stream."""
    return _decompress_batch_device(1, d_in, montgomery, stream)


def bn254_g2_decompress_batch_device(d_in, montgomery=False, stream=None):
    """The same for G2: uint8 cuda [n, 64] -> ([n, 128], status).  Subgroup membership is not looked at."""
    return _decompress_batch_device(2, d_in, montgomery, stream)


def groth16_compress_proofs_device(d_proofs, stream=None):
    """Device proofs (uint8 cuda [B, 256], the prover's layout) -> a uint8 cuda tensor [B, 128]: A (32), B (64), C (32) compressed.
    Asynchronous on `stream` or the current torch stream."""
    import torch
    b = _codec_args(d_proofs, GROTH16_PROOF_BYTES)
    out = torch.empty((b, GROTH16_CPROOF_BYTES), dtype=torch.uint8, device=d_proofs.device)
    with _device_call(d_proofs, stream, (d_proofs, out)) as s:
        _r1cs_call(r1cs_lib().gwb_groth16_proofs_compress_device, d_proofs.data_ptr() if b else None, b, out.data_ptr() if b else None, s.cuda_stream)
    return out


def groth16_decompress_proofs_device(d_cproofs, stream=None):
    """Compressed device proofs (uint8 cuda [B, 128]) -> (proofs [B, 256], status int32 [B]): VERIFY_POINT when any of A, B, C was
    refused (that point is then (0, 0)), else VERIFY_VALID.  Asynchronous on `stream` or the current torch stream."""
    import torch
    b = _codec_args(d_cproofs, GROTH16_CPROOF_BYTES)
    out = torch.empty((b, GROTH16_PROOF_BYTES), dtype=torch.uint8, device=d_cproofs.device)
    status = torch.empty(b, dtype=torch.int32, device=d_cproofs.device)
    with _device_call(d_cproofs, stream, (d_cproofs, out, status)) as s:
        _r1cs_call(r1cs_lib().gwb_groth16_proofs_decompress_device, d_cproofs.data_ptr() if b else None, b, out.data_ptr() if b else None,
                   status.data_ptr() if b else None, s.cuda_stream)
    return out, status


def groth16_compress_proofs(proofs):
    """Host proofs uint8 [B, 256] -> uint8 [B, 128], on the GPU.  Synchronous."""
    import torch
    p = np.array(proofs, dtype=np.uint8).reshape(-1, GROTH16_PROOF_BYTES)
    return groth16_compress_proofs_device(torch.from_numpy(p).cuda()).cpu().numpy()


def groth16_decompress_proofs(cproofs):
    """Host compressed proofs uint8 [B, 128] -> (proofs uint8 [B, 256], status uint32 [B]), on the GPU.  Synchronous."""
    import torch
    p = np.array(cproofs, dtype=np.uint8).reshape(-1, GROTH16_CPROOF_BYTES)
    out, status = groth16_decompress_proofs_device(torch.from_numpy(p).cuda())
    return out.cpu().numpy(), status.cpu().numpy().astype(np.uint32)


# -- KZG commitments over a powers-of-tau file (include/graph_witness_kzg.h, libcwc_r1cs.so) ----------------------------------------
KZG_VALID, KZG_SCALAR, KZG_POINT, KZG_EQUATION = 0, 1, 2, 3
KZG_CHECK_POWERS = 1
KZG_PHASES = ("quotient", "lincomb", "prepare", "pairing")
KZG_FOLD_PHASES = ("fold", "evals", "quotient", "lincomb", "prepare", "pairing")


def _kzg_host(a, tail, what):
    """a host array as contiguous uint8 [K, *tail]; the last dimensions have to be `tail` already (-1: any length)"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != 1 + len(tail) or any(t != -1 and t != d for t, d in zip(tail, a.shape[1:])):
        raise WitnessCalcError("kzg: %s: uint8 [K, %s] expected, got %s" % (what, ", ".join("N" if t == -1 else str(t) for t in tail), list(a.shape)))
    return a


def _kzg_dev(t, tail, what, k=None):
    import torch
    ok = hasattr(t, "is_cuda") and t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8 and t.dim() == 1 + len(tail)
    ok = ok and all(e == -1 or e == d for e, d in zip(tail, t.shape[1:])) and (k is None or t.shape[0] == k)
    if not ok:
        raise WitnessCalcError("kzg: %s: a contiguous uint8 cuda tensor [K, %s] expected" % (what, ", ".join("N" if e == -1 else str(e) for e in tail)))
    return t


def _kzg_shaped(a, shape, what, device=False, g=None):
    """A folded call's array: contiguous uint8 of `shape`, whose names stand for any length and whose numbers for themselves; the
    first dimension is g when that is given.  A host array, or with `device` a cuda tensor."""
    if device:
        import torch
        ok = hasattr(a, "is_cuda") and a.is_cuda and a.is_contiguous() and a.dtype == torch.uint8
    else:
        a = np.ascontiguousarray(a, dtype=np.uint8)
        ok = True
    ok = ok and len(a.shape) == len(shape) and all(isinstance(e, str) or e == d for e, d in zip(shape, a.shape)) and (g is None or a.shape[0] == g)
    if not ok:
        want = "[%s]" % ", ".join(str(e) for e in shape)
        if device:
            raise WitnessCalcError("kzg: %s: a contiguous uint8 cuda tensor %s expected" % (what, want))
        raise WitnessCalcError("kzg: %s: uint8 %s expected, got %s" % (what, want, list(a.shape)))
    return a


def _kzg_log2(n, what):
    if n < 1 or n & (n - 1):
        raise WitnessCalcError("kzg: %s: %d evaluations, a power of two expected" % (what, n))
    return n.bit_length() - 1


class Kzg(_Handle):
    """KZG polynomial commitments over a `.ptau` image (bytes or any buffer, an mmap included; it is not kept): commit to
    polynomials given by coefficients or by evaluations, open them at points, check openings.  max_len: the longest polynomial,
    in coefficients (default: every point of the file, 2^(power+1) - 1).  check_powers: run ptau_check_powers' rule over the
    covered prefix first.  The SRS is whatever the file holds: check_powers and ptau_verify are what vouch for it.  Scalars are
    32 bytes little-endian, points 64 bytes canonical affine (zero bytes: infinity).  The plain methods take and return numpy
    arrays and are synchronous; the _device methods take torch cuda tensors and are asynchronous on `stream` or the current
    stream."""
    _FREE = ("_r1cs_lib", "gwb_kzg_free")

    def __init__(self, ptau, max_len=None, check_powers=False):
        keep, addr, n = _ptau_buffer(ptau)
        if max_len is None:
            max_len = (2 << ptau_info(ptau)["power"]) - 1
        if int(max_len) < 0 or int(max_len) >= 1 << 64:
            raise WitnessCalcError("kzg: max_len %d" % max_len)
        self._h = ctypes.c_void_p()
        _r1cs_call(r1cs_lib().gwb_kzg_new, addr, n, int(max_len), KZG_CHECK_POWERS if check_powers else 0, ctypes.byref(self._h))
        info = KzgInfo()
        r1cs_lib().gwb_kzg_info(self._h, ctypes.byref(info))
        self.info = {"max_len": int(info.max_len), "power": int(info.power), "prepared": bool(info.prepared)}

    def commit(self, polys):
        """uint8 [K, N, 32] -> commitments uint8 [K, 64]"""
        p = _kzg_host(polys, (-1, 32), "polys")
        out = np.zeros((p.shape[0], 64), dtype=np.uint8)
        _r1cs_call(r1cs_lib().gwb_kzg_commit_batch, self._h, p.ctypes.data, p.shape[0], p.shape[1], out.ctypes.data)
        return out

    def commit_device(self, d_polys, stream=None):
        import torch
        p = _kzg_dev(d_polys, (-1, 32), "d_polys")
        out = torch.empty((p.shape[0], 64), dtype=torch.uint8, device=p.device)
        with _device_call(p, stream, (p, out)) as s:
            _r1cs_call(r1cs_lib().gwb_kzg_commit_batch_device, self._h, p.data_ptr(), p.shape[0], p.shape[1], out.data_ptr(), s.cuda_stream)
        return out

    def commit_evals(self, evals):
        """uint8 [K, 2^m, 32], the evaluations at the powers of the domain's root in natural order -> commitments uint8 [K, 64]
        (the file has to be prepared: ptau_prepare_phase2)"""
        e = _kzg_host(evals, (-1, 32), "evals")
        m = _kzg_log2(e.shape[1], "evals")
        out = np.zeros((e.shape[0], 64), dtype=np.uint8)
        _r1cs_call(r1cs_lib().gwb_kzg_commit_evals_batch, self._h, e.ctypes.data, e.shape[0], m, out.ctypes.data)
        return out

    def commit_evals_device(self, d_evals, stream=None):
        import torch
        e = _kzg_dev(d_evals, (-1, 32), "d_evals")
        m = _kzg_log2(e.shape[1], "d_evals")
        out = torch.empty((e.shape[0], 64), dtype=torch.uint8, device=e.device)
        with _device_call(e, stream, (e, out)) as s:
            _r1cs_call(r1cs_lib().gwb_kzg_commit_evals_batch_device, self._h, e.data_ptr(), e.shape[0], m, out.data_ptr(), s.cuda_stream)
        return out

    def eval(self, polys, zs):
        """uint8 [K, N, 32] and points uint8 [K, 32] -> values uint8 [K, 32]"""
        p = _kzg_host(polys, (-1, 32), "polys")
        z = _kzg_host(zs, (32,), "zs")
        if z.shape[0] != p.shape[0]:
            raise WitnessCalcError("kzg: %d polynomials and %d points" % (p.shape[0], z.shape[0]))
        ys = np.zeros((p.shape[0], 32), dtype=np.uint8)
        _r1cs_call(r1cs_lib().gwb_kzg_eval_batch, self._h, p.ctypes.data, z.ctypes.data, p.shape[0], p.shape[1], ys.ctypes.data)
        return ys

    def open(self, polys, zs):
        """uint8 [K, N, 32] and points uint8 [K, 32] -> (values uint8 [K, 32], proofs uint8 [K, 64])"""
        p = _kzg_host(polys, (-1, 32), "polys")
        z = _kzg_host(zs, (32,), "zs")
        if z.shape[0] != p.shape[0]:
            raise WitnessCalcError("kzg: %d polynomials and %d points" % (p.shape[0], z.shape[0]))
        ys, ws = np.zeros((p.shape[0], 32), dtype=np.uint8), np.zeros((p.shape[0], 64), dtype=np.uint8)
        _r1cs_call(r1cs_lib().gwb_kzg_open_batch, self._h, p.ctypes.data, z.ctypes.data, p.shape[0], p.shape[1], ys.ctypes.data, ws.ctypes.data)
        return ys, ws

    def open_device(self, d_polys, d_zs, stream=None):
        import torch
        p = _kzg_dev(d_polys, (-1, 32), "d_polys")
        z = _kzg_dev(d_zs, (32,), "d_zs", p.shape[0])
        ys = torch.empty((p.shape[0], 32), dtype=torch.uint8, device=p.device)
        ws = torch.empty((p.shape[0], 64), dtype=torch.uint8, device=p.device)
        with _device_call(p, stream, (p, z, ys, ws)) as s:
            _r1cs_call(r1cs_lib().gwb_kzg_open_batch_device, self._h, p.data_ptr(), z.data_ptr(), p.shape[0], p.shape[1], ys.data_ptr(), ws.data_ptr(),
                       s.cuda_stream)
        return ys, ws

    def verify(self, commitments, zs, ys, proofs):
        """uint8 [K, 64], [K, 32], [K, 32], [K, 64] -> uint32 [K] of KZG_VALID, KZG_SCALAR, KZG_POINT, KZG_EQUATION"""
        c = _kzg_host(commitments, (64,), "commitments")
        z, y, w = _kzg_host(zs, (32,), "zs"), _kzg_host(ys, (32,), "ys"), _kzg_host(proofs, (64,), "proofs")
        k = c.shape[0]
        if not (z.shape[0] == y.shape[0] == w.shape[0] == k):
            raise WitnessCalcError("kzg: %d commitments, %d points, %d values and %d proofs" % (k, z.shape[0], y.shape[0], w.shape[0]))
        out = np.zeros(k, dtype=np.uint32)
        _r1cs_call(r1cs_lib().gwb_kzg_verify_batch, self._h, c.ctypes.data, z.ctypes.data, y.ctypes.data, w.ctypes.data, k, out.ctypes.data)
        return out

    def verify_device(self, d_commitments, d_zs, d_ys, d_proofs, stream=None):
        """-> an int32 cuda tensor [K] of statuses"""
        import torch
        c = _kzg_dev(d_commitments, (64,), "d_commitments")
        k = c.shape[0]
        z, y, w = _kzg_dev(d_zs, (32,), "d_zs", k), _kzg_dev(d_ys, (32,), "d_ys", k), _kzg_dev(d_proofs, (64,), "d_proofs", k)
        out = torch.empty(k, dtype=torch.int32, device=c.device)
        with _device_call(c, stream, (c, z, y, w, out)) as s:
            _r1cs_call(r1cs_lib().gwb_kzg_verify_batch_device, self._h, c.data_ptr(), z.data_ptr(), y.data_ptr(), w.data_ptr(), k, out.data_ptr(), s.cuda_stream)
        return out


    # -- folded openings: G groups of K polynomials, one point, one challenge gamma and one witness per group
    def open_fold(self, polys, zs, gammas):
        """uint8 [G, K, N, 32], points [G, 32] and challenges [G, 32] -> (values uint8 [G, K, 32], proofs uint8 [G, 64]): y_k =
        p_k(z) and the one witness of sum_k gamma^k p_k at z.  gamma is the caller's protocol challenge; the check binds each y_k
        to its commitment only if gamma was fixed after the commitments, z and the y_k."""
        p = _kzg_shaped(polys, ("G", "K", "N", 32), "polys")
        g, k, n = p.shape[:3]
        z, gm = _kzg_shaped(zs, ("G", 32), "zs"), _kzg_shaped(gammas, ("G", 32), "gammas")
        if not (z.shape[0] == gm.shape[0] == g):
            raise WitnessCalcError("kzg: %d groups, %d points and %d challenges" % (g, z.shape[0], gm.shape[0]))
        ys, ws = np.zeros((g, k, 32), dtype=np.uint8), np.zeros((g, 64), dtype=np.uint8)
        _r1cs_call(r1cs_lib().gwb_kzg_open_fold_batch, self._h, p.ctypes.data, z.ctypes.data, gm.ctypes.data, g, k, n, ys.ctypes.data, ws.ctypes.data)
        return ys, ws

    def open_fold_device(self, d_polys, d_zs, d_gammas, stream=None):
        import torch
        p = _kzg_shaped(d_polys, ("G", "K", "N", 32), "d_polys", device=True)
        g, k, n = p.shape[:3]
        z, gm = _kzg_shaped(d_zs, ("G", 32), "d_zs", device=True, g=g), _kzg_shaped(d_gammas, ("G", 32), "d_gammas", device=True, g=g)
        ys = torch.empty((g, k, 32), dtype=torch.uint8, device=p.device)
        ws = torch.empty((g, 64), dtype=torch.uint8, device=p.device)
        with _device_call(p, stream, (p, z, gm, ys, ws)) as s:
            _r1cs_call(r1cs_lib().gwb_kzg_open_fold_batch_device, self._h, p.data_ptr(), z.data_ptr(), gm.data_ptr(), g, k, n, ys.data_ptr(), ws.data_ptr(),
                       s.cuda_stream)
        return ys, ws

    def verify_fold(self, commitments, zs, gammas, ys, proofs):
        """uint8 [G, K, 64], [G, 32], [G, 32], [G, K, 32], [G, 64] -> uint32 [G] of KZG_VALID, KZG_SCALAR, KZG_POINT, KZG_EQUATION:
        e(sum_k gamma^k C_k - (sum_k gamma^k y_k) G1 + z W, G2) = e(W, tauG2) per group"""
        c = _kzg_shaped(commitments, ("G", "K", 64), "commitments")
        g, k = c.shape[:2]
        z, gm, w = _kzg_shaped(zs, ("G", 32), "zs"), _kzg_shaped(gammas, ("G", 32), "gammas"), _kzg_shaped(proofs, ("G", 64), "proofs")
        y = _kzg_shaped(ys, ("G", "K", 32), "ys")
        if not (z.shape[0] == gm.shape[0] == w.shape[0] == y.shape[0] == g) or y.shape[1] != k:
            raise WitnessCalcError("kzg: %d groups of %d commitments, %d points, %d challenges, %d groups of %d values and %d proofs" %
                                   (g, k, z.shape[0], gm.shape[0], y.shape[0], y.shape[1], w.shape[0]))
        out = np.zeros(g, dtype=np.uint32)
        _r1cs_call(r1cs_lib().gwb_kzg_verify_fold_batch, self._h, c.ctypes.data, z.ctypes.data, gm.ctypes.data, y.ctypes.data, w.ctypes.data, g, k,
                   out.ctypes.data)
        return out

    def verify_fold_device(self, d_commitments, d_zs, d_gammas, d_ys, d_proofs, stream=None):
        """-> an int32 cuda tensor [G] of statuses"""
        import torch
        c = _kzg_shaped(d_commitments, ("G", "K", 64), "d_commitments", device=True)
        g, k = c.shape[:2]
        z, gm = _kzg_shaped(d_zs, ("G", 32), "d_zs", device=True, g=g), _kzg_shaped(d_gammas, ("G", 32), "d_gammas", device=True, g=g)
        y, w = _kzg_shaped(d_ys, ("G", "K", 32), "d_ys", device=True, g=g), _kzg_shaped(d_proofs, ("G", 64), "d_proofs", device=True, g=g)
        if y.shape[1] != k:
            raise WitnessCalcError("kzg: %d commitments and %d values per group" % (k, y.shape[1]))
        out = torch.empty(g, dtype=torch.int32, device=c.device)
        with _device_call(c, stream, (c, z, gm, y, w, out)) as s:
            _r1cs_call(r1cs_lib().gwb_kzg_verify_fold_batch_device, self._h, c.data_ptr(), z.data_ptr(), gm.data_ptr(), y.data_ptr(), w.data_ptr(), g, k,
                       out.data_ptr(), s.cuda_stream)
        return out


def kzg_fold_device(d_polys, d_gammas, stream=None):
    """Test and measurement aid of the fold kernel: uint8 cuda [G, K, N, 32] and [G, 32] -> [G, N, 32], sum_k gamma^k p_k per group,
    canonical.  Asynchronous on `stream` or the current stream."""
    import torch
    p = _kzg_shaped(d_polys, ("G", "K", "N", 32), "d_polys", device=True)
    g, k, n = p.shape[:3]
    gm = _kzg_shaped(d_gammas, ("G", 32), "d_gammas", device=True, g=g)
    out = torch.empty((g, n, 32), dtype=torch.uint8, device=p.device)
    with _device_call(p, stream, (p, gm, out)) as s:
        _r1cs_call(r1cs_lib().gwb_kzg_fold_device, p.data_ptr(), gm.data_ptr(), g, k, n, out.data_ptr(), s.cuda_stream)
    return out


def kzg_fold_points_device(d_points, d_gammas, stream=None):
    """Test and measurement aid of the verifier's point fold: uint8 cuda [G, K, 64] and [G, 32] -> [G, 64], sum_k gamma^k C_k per
    group.  A point with a coordinate at or above q or off the curve is refused; to say so the call waits for the stream."""
    import torch
    c = _kzg_shaped(d_points, ("G", "K", 64), "d_points", device=True)
    g, k = c.shape[:2]
    gm = _kzg_shaped(d_gammas, ("G", 32), "d_gammas", device=True, g=g)
    out = torch.empty((g, 64), dtype=torch.uint8, device=c.device)
    with _device_call(c, stream, (c, gm, out)) as s:
        _r1cs_call(r1cs_lib().gwb_kzg_fold_points_device, c.data_ptr(), gm.data_ptr(), g, k, out.data_ptr(), s.cuda_stream)
    return out


def kzg_fold_phase_ms(k):
    """{fold, evals, quotient, lincomb, prepare, pairing} in ms of the handle's last open_fold or verify_fold call (waits for it)."""
    return _phase_ms(r1cs_lib().gwb_kzg_fold_phase_ms, KZG_FOLD_PHASES, "no KZG fold phase times (no open_fold or verify_fold call yet)", k._h)


def kzg_tiles():
    """The tile sizes (coefficients per workgroup) of the evaluate-and-quotient kernels, smallest first; the last is production's."""
    n = ctypes.c_size_t(8)
    tiles = (ctypes.c_uint32 * 8)()
    if r1cs_lib().gwb_kzg_tiles(tiles, ctypes.byref(n)) != 0:
        raise WitnessCalcError("gwb_kzg_tiles failed")
    return [int(tiles[i]) for i in range(n.value)]


def kzg_eval_quotient_device(d_polys, d_zs, tile=None, stream=None):
    """Test and measurement aid of the evaluate-and-quotient kernels: uint8 cuda [K, N, 32] and [K, 32] -> (d_ys [K, 32],
    d_qs [K, N - 1, 32]), y = p(z) and the coefficients of (p(X) - y) / (X - z), with workgroups of `tile` coefficients (one of
    kzg_tiles(); None: production's).  Asynchronous on `stream` or the current stream."""
    import torch
    p = _kzg_dev(d_polys, (-1, 32), "d_polys")
    k, n = p.shape[0], p.shape[1]
    z = _kzg_dev(d_zs, (32,), "d_zs", k)
    ys = torch.empty((k, 32), dtype=torch.uint8, device=p.device)
    qs = torch.empty((k, max(n - 1, 0), 32), dtype=torch.uint8, device=p.device)
    with _device_call(p, stream, (p, z, ys, qs)) as s:
        _r1cs_call(r1cs_lib().gwb_kzg_eval_quotient_device, p.data_ptr(), z.data_ptr(), k, n, 0 if tile is None else int(tile), ys.data_ptr(), qs.data_ptr(),
                   s.cuda_stream)
    return ys, qs


def kzg_phase_ms(k):
    """{quotient, lincomb, prepare, pairing} in ms of the handle's last open or verify call (waits for it)."""
    return _phase_ms(r1cs_lib().gwb_kzg_phase_ms, KZG_PHASES, "no KZG phase times (no open or verify call yet)", k._h)


from . import graphgen  # noqa: E402,F401  (graph generator library on top of the C-ABI producer)
