"""Groth16 witness map of the authV2-class graph (include/graph_witness_r1cs.h, gwb_r1cs_qap_*) at 1, 64 and 1 024 sets: HIP-event
times of the whole call and per phase (evaluation; inverse outer passes; the fused inner pass = inverse, coset scaling and
forward; forward outer passes with A B - C), a bytes model and its fraction of 8 TB/s, the Montgomery-product count and its
fraction of the chip's measured modmul rate, and the 1 024-set total against the witness step, timed the same way on the same
box.  The R1CS is derived from the generator's circuit (tests/r1cs_fixtures.py).  Writes the report to stdout and to the path
given as the first argument, if any.

The phase times come from a run with the workspace cap raised (CWC_R1CS_QAP_WORKSPACE_MB, set below before the library is
loaded) so that 1 024 sets are one sub-batch; the default cap splits them in two."""
import os
import sys
import time

os.environ.setdefault("CWC_R1CS_QAP_WORKSPACE_MB", "16384")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cwc_import  # noqa: E402
from tests import r1cs_fixtures as F  # noqa: E402
from tools.synth import synth_inputs  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
BATCHES, REPS = (1, 64, 1024), 10
PHASES = ("evaluation", "inverse_outer", "fused_inner", "forward_outer")
LOG_TILE, LOG_OUTER_MAX = 11, 9  # r1cs/qap.hip's pass plan


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def plan(p):
    inner = min(p, LOG_TILE)
    rest = p - inner
    m = (rest + LOG_OUTER_MAX - 1) // LOG_OUTER_MAX
    return [rest // m + (1 if t < rest % m else 0) for t in range(m)] + [inner]


def models(info, n_fac_ab, n_general_ab, p):
    """per set: (bytes by phase, Montgomery products by phase)"""
    n = 1 << p
    ls = plan(p)
    m = len(ls) - 1
    e = 32
    byts = {"evaluation": n_fac_ab * e + 3 * n * e,           # witness gathers of A and B; a, b, c written
            "inverse_outer": m * 6 * n * e,                   # 3 arrays read and written per pass
            "fused_inner": 6 * n * e,
            "forward_outer": max(m - 1, 0) * 6 * n * e + (4 * n * e if m else 0)}  # the last pass writes h only
    if not m:
        byts["fused_inner"] = 4 * n * e
    nc = info["n_constraints"]
    dft = lambda l: (n // 2) * (l - 1)  # the first stage of a pass needs no product
    mul = {"evaluation": n_general_ab + 3 * nc,               # general factors; a, b to Montgomery; c = a b
           "inverse_outer": 3 * sum(dft(l) + n for l in ls[:-1]),
           "fused_inner": 3 * (2 * dft(ls[-1]) + n),
           "forward_outer": 3 * sum(dft(l) + n for l in ls[:-1])}
    last = "forward_outer" if m else "fused_inner"
    mul[last] += 2 * n  # A B and the conversion to canonical
    return byts, mul


def main():
    pkg = cwc_import.load()
    C = pkg.graphgen.circuits
    t0 = time.time()
    with F.gadget_constraints():
        b = C.build_authv2_class()
    cons = F.derive_r1cs(b)
    g = pkg.Graph(b.to_bin())
    r = pkg.R1cs(F.write_r1cs(len(b._witness), cons))
    info, qi = r.info, r.qap_info()
    p = qi["domain_power"]
    n_fac_ab = info["n_factors_a"] + info["n_factors_b"]
    n_general_ab = sum(1 for con in cons for lc in con[:2] for c in lc.values() if c not in (1, F.R - 1))
    setup_s = time.time() - t0
    rate = pkg.modmul_rate()
    lines = ["Groth16 witness map (QAP h), authV2-class graph (build_authv2_class(), R1CS derived by tests/r1cs_fixtures.py)",
             "circuit: %d wires, %d constraints, %d A+B factors (%d with a general coefficient); N = %d rows, domain 2^%d = %d, "
             "pass plan (log L, outermost first) %s" % (info["n_wires"], info["n_constraints"], n_fac_ab, n_general_ab, qi["n_rows"], p,
                                                        qi["domain_size"], plan(p)),
             "setup (graph build + derivation, host): %.1f s" % setup_s,
             "measured modmul rate (probe kernel, dependent fr_mul chains, 8 waves/SIMD): %.1f G products/s" % (rate / 1e9),
             "workspace cap for the phase runs: CWC_R1CS_QAP_WORKSPACE_MB=%s (%d MiB per set)" % (
                 os.environ["CWC_R1CS_QAP_WORKSPACE_MB"], qi["workspace_bytes_per_row"] >> 20)]
    byts, mul = models(info, n_fac_ab, n_general_ab, p)
    step_ms = None
    ok = True
    for batch in BATCHES:
        d_in = torch.from_numpy(synth_inputs("field", g.n_inputs, batch, 31)).cuda()
        d_w = torch.empty((batch, g.n_witness, 32), dtype=torch.uint8, device="cuda")
        d_st = torch.zeros(batch, dtype=torch.int32, device="cuda")
        step = lambda: g.calc_witness_batch_device(d_in, d_w, d_st)
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        s_ms, _ = timed(step, REPS)
        res = {}
        fn = lambda: res.__setitem__("h", r.qap_batch_device(d_w))
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ms, ms_min = timed(fn, REPS)
        # correctness spot check: set 0 against the host path
        h0 = res["h"][:1].cpu().numpy()
        ok &= bool((r.qap_batch(d_w[:1].cpu().numpy()) == h0).all())
        r.qap_time_phases(True)
        phase = {k: [] for k in PHASES}
        for _ in range(5):
            r.qap_batch_device(d_w)
            for k, v in r.qap_phase_ms().items():
                phase[k].append(v)
        r.qap_time_phases(False)
        phase = {k: float(np.median(v)) for k, v in phase.items()}
        tot_b = sum(byts.values()) * batch
        tot_m = sum(mul.values()) * batch
        lines.append("")
        lines.append("batch %d: qap_batch_device median %.3f ms, min %.3f ms over %d calls; witness step median %.3f ms; qap = %.0f %% of the "
                     "witness step" % (batch, ms, ms_min, REPS, s_ms, 100 * ms / s_ms))
        lines.append("  total: bytes model %.3f GB -> %.2f TB/s, %.1f %% of 8 TB/s; %.3f G Montgomery products -> %.1f G/s, %.1f %% of the "
                     "measured modmul rate" % (tot_b / 1e9, tot_b / (ms * 1e-3) / 1e12, 100 * tot_b / (ms * 1e-3) / HBM_BYTES_PER_S,
                                               tot_m / 1e9, tot_m / (ms * 1e-3) / 1e9, 100 * tot_m / (ms * 1e-3) / rate))
        for k in PHASES:
            t = phase[k]
            bb, mm = byts[k] * batch, mul[k] * batch
            if t > 0:
                lines.append("  %-14s %8.3f ms (%4.1f %%): bytes %.3f GB -> %.1f %% of 8 TB/s; products %.3f G -> %.1f %% of the modmul rate" % (
                    k, t, 100 * t / sum(phase.values()), bb / 1e9, 100 * bb / (t * 1e-3) / HBM_BYTES_PER_S, mm / 1e9,
                    100 * mm / (t * 1e-3) / rate))
            else:
                lines.append("  %-14s %8.3f ms (no pass at this domain)" % (k, t))
        if batch == 1024:
            step_ms = s_ms
            total_1024 = ms
        del d_w, res
        torch.cuda.empty_cache()
    lines.append("")
    lines.append("1 024 sets: witness map %.3f ms against the witness step's %.3f ms (%.2f x)" % (total_1024, step_ms, total_1024 / step_ms))
    lines.append("spot checks (set 0 of each batch, device against host path): %s" % ("ok" if ok else "MISMATCH"))
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
