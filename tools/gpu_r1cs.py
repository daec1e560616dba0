"""R1CS check of the authV2-class graph at 1 024 sets (include/graph_witness_r1cs.h): the check kernel's time from HIP events, its
bytes model (batch x sum of factors x 32 B of witness gathers + the constraint stream), that model's fraction of 8 TB/s, and the
witness step it screens, timed the same way on the same box.  The R1CS is derived from the generator's circuit
(tests/r1cs_fixtures.py).  Writes the report to stdout and to the path given as the first argument, if any."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cwc_import  # noqa: E402
from tests import r1cs_fixtures as F  # noqa: E402
from tools.synth import synth_inputs  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
BATCH, REPS = 1024, 20


def timed(fn, reps):
    """median ms of `reps` calls of fn() on the current stream, each between two HIP events"""
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    pkg = cwc_import.load()
    C = pkg.graphgen.circuits
    t0 = time.time()
    with F.gadget_constraints():
        b = C.build_authv2_class()
    cons = F.derive_r1cs(b)
    g = pkg.Graph(b.to_bin())
    r = pkg.R1cs(F.write_r1cs(len(b._witness), cons))
    info = r.info
    n_fac = info["n_factors_a"] + info["n_factors_b"] + info["n_factors_c"]
    n_general = sum(1 for con in cons for lc in con for c in lc.values() if c not in (1, F.R - 1))
    setup_s = time.time() - t0
    d_in = torch.from_numpy(synth_inputs("field", g.n_inputs, BATCH, 31)).cuda()
    d_w = torch.empty((BATCH, g.n_witness, 32), dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(BATCH, dtype=torch.int32, device="cuda")
    step = lambda: g.calc_witness_batch_device(d_in, d_w, d_st)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    step_ms, step_min = timed(step, REPS)
    lines = ["R1CS check, authV2-class graph (build_authv2_class(), R1CS derived by tests/r1cs_fixtures.py), %d sets" % BATCH,
             "circuit: %d wires, %d constraints, %d factors (A %d, B %d, C %d; %d with a general coefficient, the rest +-1), "
             "%d distinct general coefficients" % (info["n_wires"], info["n_constraints"], n_fac, info["n_factors_a"], info["n_factors_b"],
                                                   info["n_factors_c"], n_general, len({c for con in cons for lc in con for c in lc.values()})),
             "setup (graph build + derivation, host): %.1f s" % setup_s,
             "witness step (calc_witness_batch_device, %d sets): median %.3f ms, min %.3f ms over %d steps" % (BATCH, step_ms, step_min, REPS)]
    first_res = None
    for t in (0, 64, 32, 8, 1):
        r.set_tile_width(t)
        res = {}
        fn = lambda: res.__setitem__("r", r.check_batch_device(d_w))
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ms, ms_min = timed(fn, REPS if t in (0, 64) else 5)
        f, n = res["r"]
        f, n = f.cpu().numpy().view(np.uint32), n.cpu().numpy()
        ok = bool((f == 0xFFFFFFFF).all() and (n == 0).all())
        stream_bytes = 4 * (3 * info["n_constraints"] + 1) + 8 * n_fac + 4 * info["n_constraints"]
        model = BATCH * n_fac * 32 + stream_bytes
        frac = model / (ms * 1e-3) / HBM_BYTES_PER_S
        lines.append("check tile width %s: median %.3f ms, min %.3f ms (%s); bytes model %d x %d x 32 + %d = %.3f GB -> %.2f TB/s, %.1f %% of 8 TB/s; "
                     "%.1f %% of the witness step" % (t or "auto (64)", ms, ms_min, "all satisfied" if ok else "NOT all satisfied", BATCH, n_fac,
                                                        stream_bytes, model / 1e9, model / (ms * 1e-3) / 1e12, 100 * frac, 100 * ms / step_ms))
        if t == 0:
            first_res = (ms, ok)
    lines.append("yardstick (not a gate): check <= 1/4 of the witness step: %s" % ("met" if first_res[0] <= step_ms / 4 else "NOT met"))
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(text + "\n")
    return 0 if first_res[1] else 1


if __name__ == "__main__":
    sys.exit(main())
