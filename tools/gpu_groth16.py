"""Groth16 proofs of the authV2-class graph (include/graph_witness_groth16.h, gwb_groth16_*) at 1, 64 and 1 024 sets: HIP-event
times of the whole call (warm) and per phase (witness map; scalar preparation and sort; G1 MSMs A, B1, C, H; G2 MSM B2;
assembly), the witness step timed the same way on the same box, and the count of curve additions and Fq products over the
measured modmul rate.  The R1CS is derived from the generator's circuit as in tools/gpu_r1cs_qap.py; the zkey is the known-log
zkey of tests/groth16_fixtures.py (arithmetic progressions: MSM cost depends on the scalars, not on the bases' discrete logs).
Writes the report to stdout and to the path given as the first argument, if any.

Fq's Montgomery product has Fr's instruction sequence (tools/codegen/gen_fq_mul.py), so gwb_r1cs_modmul_rate's probe rate is
used for both."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cwc_import  # noqa: E402
from tests import groth16_fixtures as GF  # noqa: E402
from tests import r1cs_fixtures as F  # noqa: E402
from tools.synth import synth_inputs  # noqa: E402

BATCHES = (1, 64, 1024)


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


def window_bits(n_sc):
    """msm.hip's window width and window count for n_sc scalars per row"""
    lg = n_sc.bit_length() - 1
    c = min(15, max(7, lg - 3))
    return c, 254 // c + 1


def main():
    pkg = cwc_import.load()
    C = pkg.graphgen.circuits
    with F.gadget_constraints():
        b = C.build_authv2_class()
    cons = F.derive_r1cs(b)
    g = pkg.Graph(b.to_bin())
    r1 = pkg.R1cs(F.write_r1cs(len(b._witness), cons))
    nv, n = r1.info["n_wires"], r1.qap_info()["domain_size"]
    t0 = time.time()
    K = GF.KnownLog(nv, 0, n)
    pr = pkg.Groth16(K.zkey, r1)
    lines = ["Groth16 proofs, authV2-class graph (build_authv2_class(), R1CS derived by tests/r1cs_fixtures.py), known-log zkey "
             "(tests/groth16_fixtures.py, %.1f MB, built in %.0f s on the host)" % (len(K.zkey) / 1e6, time.time() - t0),
             "circuit: %d wires, %d constraints, domain %d; MSMs per proof: A, B1 (G1, nVars + 2), C (G1, nVars - 1), B2 (G2, "
             "nVars + 2), H (G1, n)" % (nv, r1.info["n_constraints"], n)]
    rate = pkg.modmul_rate()
    lines.append("modmul probe: %.3g Montgomery products / s (Fq's product has Fr's instruction shape)" % rate)
    d_st = None
    for batch in BATCHES:
        d_in = torch.from_numpy(synth_inputs("field", g.n_inputs, batch, 41)).cuda()
        d_w = torch.empty((batch, g.n_witness, 32), dtype=torch.uint8, device="cuda")
        d_st = torch.zeros(batch, dtype=torch.int32, device="cuda")
        reps = 5 if batch < 1024 else 2
        wit = timed(lambda: g.calc_witness_batch_device(d_in, d_w, d_st), reps)
        assert not d_st.cpu().numpy().any()
        rs = [(1 + i, 2 + i) for i in range(batch)]
        pr.prove_batch_device(d_w, rs=rs)  # warm-up: uploads, workspace
        torch.cuda.synchronize()
        call = timed(lambda: pr.prove_batch_device(d_w, rs=rs), reps)
        pr.time_phases(True)
        pr.prove_batch_device(d_w, rs=rs)
        ph = pr.phase_ms()
        pr.time_phases(False)
        lines.append("batch %4d: prove %.2f ms per call (median of %d, min %.2f), %.3f ms per proof; witness step %.2f ms per call; "
                     "phases of the last sub-batch (ms): %s" % (batch, call[0], reps, call[1], call[0] / batch, wit[0],
                                                                ", ".join("%s %.2f" % kv for kv in ph.items())))
    # operation counts per proof (random-looking scalars: every digit nonzero), against the probe's rate
    cw, ww = window_bits(nv + 2)
    ch, wh = window_bits(n)
    adds_g1 = ww * (2 * (nv + 2) + (nv - 1)) + wh * n
    adds_g2 = ww * (nv + 2)
    fq_products = adds_g1 * 11 + adds_g2 * 33  # mixed XYZZ addition: 8 products + 3 squares (Fq2: 3 + 2 Fq products each)
    lines.append("model per proof (every digit nonzero): %d G1 and %d G2 mixed additions in the bucket accumulation, %.3g Fq "
                 "products, %.2f ms at the probe's rate; not modelled: bucket reduction, sort, witness map" %
                 (adds_g1, adds_g2, fq_products, fq_products / rate * 1e3))
    lines.append("not measured: a reference prover (none exists on the GPU machine); zkeys written by snarkjs (none available); witnesses of bits "
                 "(synth inputs give field-sized wires where the circuit computes them)")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out)


if __name__ == "__main__":
    main()
