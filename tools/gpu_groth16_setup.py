"""Groth16 key setup of the authV2-class circuit on the GPU (include/graph_witness_groth16_setup.h, gwb_groth16_setup): the time
of the whole call (host clock around the synchronous call: transpose, device work, file assembly) and of its five device phases
(HIP events), the column sums with split and with unsplit columns, the fixed-base multiplication rates of both groups, and then
the real chain at that size: 64 witness rows proved with the new key and checked through the pairing (all VALID), and again
with one public signal altered (all EQUATION).  The R1CS is derived from the generator's circuit as in tools/gpu_groth16.py,
with the circuit's first three signals declared public.  Writes the report to stdout and to the path given as the first
argument, if any."""
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

BATCH = 64
N_PUB = 3
REPS = 5
GEN_MUL_N = {1: 1 << 19, 2: 1 << 17}


def timed_setup(pkg, r1, trap, reps):
    """-> (zkey of the last call, wall seconds per call, phase ms per call)"""
    walls, phases, zkey = [], [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        zkey = pkg.groth16_setup(r1, trap)  # synchronous: returns after the device is done
        walls.append(time.perf_counter() - t0)
        phases.append(pkg.groth16_setup_phase_ms())
    return zkey, walls, phases


def median_phases(phases):
    return {k: float(np.median([p[k] for p in phases])) for k in phases[0]}


def main():
    pkg = cwc_import.load()
    C = pkg.graphgen.circuits
    with F.gadget_constraints():
        b = C.build_authv2_class()
    cons = F.derive_r1cs(b)
    g = pkg.Graph(b.to_bin())
    r1 = pkg.R1cs(F.write_r1cs(len(b._witness), cons, n_pub_in=N_PUB))
    nv, n = r1.info["n_wires"], r1.qap_info()["domain_size"]
    n_terms = r1.info["n_factors_a"] + r1.info["n_factors_b"] + r1.info["n_factors_c"]
    lines = ["Groth16 key setup, authV2-class graph (build_authv2_class(), R1CS derived by tests/r1cs_fixtures.py, %d public "
             "signals)" % N_PUB,
             "circuit: %d wires, %d constraints, %d terms (A %d, B %d, C %d), domain %d; fixed-base multiplications: %d in G1, "
             "%d in G2" % (nv, r1.info["n_constraints"], n_terms, r1.info["n_factors_a"], r1.info["n_factors_b"],
                           r1.info["n_factors_c"], n, 3 * nv - N_PUB - 1 + (N_PUB + 1) + n + 3, nv + 3)]
    trap = (0x1234567 << 200 | 5, 7 << 180 | 11, 13 << 190 | 17, 19 << 170 | 23, 29 << 210 | 31)
    pkg.groth16_setup(r1, trap)  # warm-up: tables of generator multiples, code objects
    zkey, walls, phases = timed_setup(pkg, r1, trap, REPS)
    ph = median_phases(phases)
    lines.append("setup call, warm (%d calls): %.0f ms median, %.0f ms min on the host clock (transpose of the matrices, device "
                 "work, copies, section 4 and file assembly; %.1f MB zkey)" % (REPS, np.median(walls) * 1e3, min(walls) * 1e3, len(zkey) / 1e6))
    lines.append("device phases (HIP events, median ms): %s; sum %.2f ms" % (", ".join("%s %.2f" % kv for kv in ph.items()), sum(ph.values())))
    # the column sums with unsplit columns, alternating with the default in the same process
    split, unsplit = [], []
    for _ in range(REPS):
        os.environ["CWC_GROTH16_SETUP_SEGMENT"] = "0"
        z0 = pkg.groth16_setup(r1, trap)
        unsplit.append(pkg.groth16_setup_phase_ms()["column_sums"])
        del os.environ["CWC_GROTH16_SETUP_SEGMENT"]
        z1 = pkg.groth16_setup(r1, trap)
        split.append(pkg.groth16_setup_phase_ms()["column_sums"])
        assert z0 == z1 == zkey
    lines.append("column sums, %d alternating calls each: columns split into segments of 64 terms %.2f ms median (min %.2f, max "
                 "%.2f); unsplit (CWC_GROTH16_SETUP_SEGMENT=0) %.2f ms median (min %.2f, max %.2f); the keys are identical" %
                 (REPS, np.median(split), min(split), max(split), np.median(unsplit), min(unsplit), max(unsplit)))
    # fixed-base multiplication rates (random scalars below 2^256: reduction, 32 mixed additions, conversion to affine)
    for group, count in GEN_MUL_N.items():
        d = torch.randint(0, 256, (count, 32), dtype=torch.uint8, device="cuda")
        pkg.bn254_gen_mul_batch_device(d, group)
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPS):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            pkg.bn254_gen_mul_batch_device(d, group)
            e.record()
            e.synchronize()
            ms.append(a.elapsed_time(e))
        lines.append("gen_mul G%d: %d scalars in %.2f ms median (min %.2f), %.3g multiplications / s" %
                     (group, count, np.median(ms), min(ms), count / (np.median(ms) * 1e-3)))
    # the chain at this size: witness -> proof -> verify
    pr = pkg.Groth16(zkey, r1)
    vk = pr.verifying_key()
    d_in = torch.from_numpy(synth_inputs("field", g.n_inputs, BATCH, 41)).cuda()
    d_w = torch.empty((BATCH, g.n_witness, 32), dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(BATCH, dtype=torch.int32, device="cuda")
    g.calc_witness_batch_device(d_in, d_w, d_st)
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    first, _ = r1.check_batch_device(d_w)
    d_p = pr.prove_batch_device(d_w)
    d_pub = d_w[:, 1:N_PUB + 1, :].contiguous()
    st = vk.verify_batch_device(d_p, d_pub).cpu().numpy()
    d_alt = d_pub.clone()
    d_alt[:, 1, 0] ^= 1  # the second public signal's lowest bit (the value stays below r)
    st_alt = vk.verify_batch_device(d_p, d_alt).cpu().numpy()
    torch.cuda.synchronize()
    n_sat = int((first.cpu().numpy() == -1).sum())
    lines.append("chain at n = %d: %d witness rows (%d satisfy the R1CS), proved with the new key, verify_batch_device: VALID %d / %d; "
                 "with one public signal altered: EQUATION %d / %d" %
                 (n, BATCH, n_sat, int((st == pkg.VERIFY_VALID).sum()), BATCH, int((st_alt == pkg.VERIFY_EQUATION).sum()), BATCH))
    lines.append("beside it: tools/gpu_groth16.py's known-log zkey of this size is built on the host in the time profiles/"
                 "groth16_authv2.txt records; not measured: snarkjs or arkworks on the same circuit (neither is on the GPU machine)")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out)
    assert n_sat == BATCH and (st == pkg.VERIFY_VALID).all() and (st_alt == pkg.VERIFY_EQUATION).all()


if __name__ == "__main__":
    main()
