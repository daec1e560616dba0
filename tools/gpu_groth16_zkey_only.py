"""Proving from the zkey alone against proving with the `.r1cs` (include/graph_witness_groth16.h), on the authV2-class key that
groth16_setup makes, at 1, 64 and 1 024 rows.  Both paths evaluate the same terms; the one difference is that the public rows go
through the factor stream of section 4 instead of the padding kernel, so the yardstick is the `.r1cs` path's own `witness_map`
phase in the same process.  Reported per batch: the `witness_map` phase (HIP events inside the prove call) and the whole call
(HIP events around it) of both paths, alternated call by call, with median, minimum and maximum of the repeats; then the one-off
host time of building the witness map from section 4 (the first gwb_zkey_qap_info of a fresh handle), and where the new path
loses time if its phase is slower than the other's by more than the spread.  The R1CS is derived from the generator's circuit as
in tools/gpu_groth16_setup.py, with the circuit's first three signals public.  Writes the report to stdout and to the path given
as the first argument, if any."""
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

BATCHES = (1, 64, 1024)
N_PUB = 3


def one_call(pr, d_w, rs):
    """-> (whole call ms by HIP events, witness_map phase ms)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    pr.prove_batch_device(d_w, rs=rs)
    b.record()
    b.synchronize()
    return a.elapsed_time(b), pr.phase_ms()["witness_map"]


def stats(v):
    return "%.3f (min %.3f, max %.3f)" % (float(np.median(v)), min(v), max(v))


def main():
    pkg = cwc_import.load()
    C = pkg.graphgen.circuits
    with F.gadget_constraints():
        b = C.build_authv2_class()
    cons = F.derive_r1cs(b)
    g = pkg.Graph(b.to_bin())
    r1 = pkg.R1cs(F.write_r1cs(len(b._witness), cons, n_pub_in=N_PUB))
    trap = (0x1234567 << 200 | 5, 7 << 180 | 11, 13 << 190 | 17, 19 << 170 | 23, 29 << 210 | 31)
    zkey = pkg.groth16_setup(r1, trap)
    alone, paired = pkg.Groth16(zkey), pkg.Groth16(zkey, r1)
    t0 = time.perf_counter()
    qi = alone.qap_info()  # the first use: section 4 -> factor stream, coefficients, buckets
    build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    alone.check_r1cs(r1)
    check_s = time.perf_counter() - t0
    lines = ["Groth16 proofs from the zkey alone against the .r1cs path, authV2-class graph (build_authv2_class(), R1CS derived by "
             "tests/r1cs_fixtures.py, %d public signals), key made by groth16_setup (%.1f MB)" % (N_PUB, len(zkey) / 1e6),
             "circuit: %d wires, %d constraints, domain %d; section 4: %d entries, %d rows used of %d" %
             (r1.info["n_wires"], r1.info["n_constraints"], qi["domain_size"], alone.info["n_coefs"], qi["n_rows"], qi["domain_size"]),
             "one-off host work: witness map built from section 4 in %.1f ms (first use of a handle); check_r1cs against the .r1cs in "
             "%.1f ms" % (build_s * 1e3, check_s * 1e3)]
    alone.time_phases(True)
    paired.time_phases(True)
    slower = []
    for batch in BATCHES:
        d_in = torch.from_numpy(synth_inputs("field", g.n_inputs, batch, 41)).cuda()
        d_w = torch.empty((batch, g.n_witness, 32), dtype=torch.uint8, device="cuda")
        d_st = torch.zeros(batch, dtype=torch.int32, device="cuda")
        g.calc_witness_batch_device(d_in, d_w, d_st)
        torch.cuda.synchronize()
        assert not d_st.cpu().numpy().any()
        rs = [(1 + i, 2 + i) for i in range(batch)]
        p0 = alone.prove_batch_device(d_w, rs=rs)  # warm-up: uploads, tables, workspaces; and the bytes agree
        p1 = paired.prove_batch_device(d_w, rs=rs)
        torch.cuda.synchronize()
        assert torch.equal(p0, p1)
        reps = 7 if batch < 1024 else 3
        res = {"alone": ([], []), "paired": ([], [])}
        for _ in range(reps):  # alternated: drift of the clocks or the machine lands on both
            for name, pr in (("alone", alone), ("paired", paired)):
                call, wm = one_call(pr, d_w, rs)
                res[name][0].append(call)
                res[name][1].append(wm)
        lines.append("batch %4d (%d alternated repeats; ms, median): witness_map zkey alone %s, with .r1cs %s; whole call zkey alone "
                     "%s, with .r1cs %s" % (batch, reps, stats(res["alone"][1]), stats(res["paired"][1]), stats(res["alone"][0]),
                                            stats(res["paired"][0])))
        spread = max(max(v) - min(v) for v in (res["alone"][1], res["paired"][1]))
        diff = float(np.median(res["alone"][1]) - np.median(res["paired"][1]))
        if diff > spread:
            slower.append((batch, diff, spread))
    if slower:
        # the transform is shared; what differs is the evaluation (nPublic + 1 more rows in the factor stream, two row
        # pointers per row) and the clearing of rows [n_used, n) by its own kernel
        alone.time_phases(False)
        for batch, diff, spread in slower:
            lines.append("batch %4d: the zkey-only witness_map is slower by %.3f ms, more than the spread of %.3f ms; the NTT passes "
                         "are the same launches on both paths, so the difference is in the evaluation and zeroing kernels" %
                         (batch, diff, spread))
    else:
        lines.append("at no batch is the zkey-only witness_map slower than the .r1cs path's by more than the spread of the repeats")
    lines.append("not measured: zkeys written by snarkjs (none available), a reference prover (none exists on the GPU machine)")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out)


if __name__ == "__main__":
    main()
