"""G2 subgroup membership on the GPU (r1cs/subgroup.hip, gwb_bn254_g2_check_batch_device): 2^17 points of G2 through the psi
criterion (method "fast") and through [r] P = O (method "order", the verifier's rule), alternated in one process, HIP events
around each call; then Groth16.check_g2() (host clock: upload, kernels, read-back) on the authV2-class key that
tools/gpu_groth16_setup.py makes.  Writes the report to stdout and to the path given as the first argument, if any."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cwc_import  # noqa: E402
from tests import r1cs_fixtures as F  # noqa: E402

N = 1 << 17
REPS = 5
N_PUB = 3


def main():
    pkg = cwc_import.load()
    d_k = torch.randint(0, 256, (N, 32), dtype=torch.uint8, device="cuda")
    d_pts = pkg.bn254_gen_mul_batch_device(d_k, 2)  # canonical points of G2
    ms = {"fast": [], "order": []}
    for rep in range(REPS + 1):  # the first round warms up
        for method in ms:
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            st = pkg.bn254_g2_check_batch_device(d_pts, method=method)
            e.record()
            e.synchronize()
            assert int(st.cpu().numpy().astype(np.int64).sum()) == 0
            if rep:
                ms[method].append(a.elapsed_time(e))
    fast, order = float(np.median(ms["fast"])), float(np.median(ms["order"]))
    lines = ["G2 subgroup membership, %d points of G2 (canonical form), %d alternating calls each after a warm-up" % (N, REPS),
             "method fast (psi criterion): %.2f ms median (min %.2f, max %.2f), %.3g points / s" % (fast, min(ms["fast"]), max(ms["fast"]), N / (fast * 1e-3)),
             "method order ([r] P = O):    %.2f ms median (min %.2f, max %.2f), %.3g points / s" % (order, min(ms["order"]), max(ms["order"]), N / (order * 1e-3)),
             "ratio order / fast: %.2f (by operation count: 254 doublings and 127 additions against 63 doublings and 30 additions, about 4)" % (order / fast)]
    C = pkg.graphgen.circuits
    with F.gadget_constraints():
        b = C.build_authv2_class()
    r1 = pkg.R1cs(F.write_r1cs(len(b._witness), F.derive_r1cs(b), n_pub_in=N_PUB))
    trap = (0x1234567 << 200 | 5, 7 << 180 | 11, 13 << 190 | 17, 19 << 170 | 23, 29 << 210 | 31)
    g = pkg.Groth16(pkg.groth16_setup(r1, trap))
    g.check_g2()
    walls = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.check_g2()
        walls.append(time.perf_counter() - t0)
    lines.append("Groth16.check_g2() on the authV2-class key (%d B2 points, beta2, gamma2, delta2), %d calls: %.1f ms median, %.1f ms min on the "
                 "host clock (upload of %.1f MB, kernels, read-back)" % (g.info["n_vars"], REPS, np.median(walls) * 1e3, min(walls) * 1e3,
                                                                        g.info["n_vars"] * 128 / 1e6))
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out)


if __name__ == "__main__":
    main()
