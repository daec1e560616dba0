"""Folded KZG openings on the GPU (include/graph_witness_kzg.h), one MI355X, warm, median of 3, HIP events, on a power-18 file that
the device makes (ptau_new and one contribution), polynomials of N = 2^18 coefficients; the two sides of every comparison
interleaved in one process:
  open_fold_device at G = 1 and K = 1, 4, 16 with its six phases, beside open_device on the same K polynomials as K rows (one
  witness per polynomial: the path before folded openings existed);
  kzg_fold_device at K = 16 in ms and GB/s of coefficients read, beside 8 TB/s of HBM and the time the modmul probe's rate gives
  for its K - 1 products per coefficient;
  verify_fold_device at K = 1, 16, 64 and G = 1, 1 024 groups with its phases, beside verify_device on G rows.
Each of the three steps runs in a child process of its own (`gpu_kzg_fold.py --step NAME`) under its own time limit, and the first
that fails or runs out of time ends the run: its figures and the later steps' read "not measured".  Writes the report to stdout
and to the path given as the first argument, if any."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cwc_import  # noqa: E402
from tools.gpu_kzg import ALPHA, BETA, N, POWER, REPS, TAU, scalars  # noqa: E402


def interleaved(a, b, reps=REPS):
    """([ms of a], [ms of b]): the two calls in turn, each between two events on the current stream"""
    ms = ([], [])
    for _ in range(reps):
        for call, out in zip((a, b), ms):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
    return ms


STEPS = {"open": 120, "fold": 60, "verify": 240}  # seconds
WHAT = {"open": "open_fold_device at K = 1, 4, 16 beside open_device on K rows", "fold": "kzg_fold_device at K = 16",
        "verify": "verify_fold_device at K = 1, 16, 64 and G = 1, 1 024 beside verify_device on G rows"}


def setup():
    pkg = cwc_import.load()
    ptau, _ = pkg.ptau_contribute(pkg.ptau_new(POWER), secrets=(TAU, ALPHA, BETA))
    return pkg, pkg.Kzg(ptau, max_len=N)


def step_open():
    """open_fold beside K single-row openings"""
    pkg, k = setup()
    lines = []
    polys = torch.from_numpy(scalars(16 * N, 1).reshape(1, 16, N, 32)).cuda()
    d_z, d_g = torch.from_numpy(scalars(1, 2)).cuda(), torch.from_numpy(scalars(1, 3)).cuda()
    for K in (1, 4, 16):
        d_p = polys[:, :K].contiguous()
        d_rows, d_zs = d_p[0].contiguous(), d_z.expand(K, 32).contiguous()
        phases = []

        def folded():
            out = k.open_fold_device(d_p, d_z, d_g)
            phases.append(pkg.kzg_fold_phase_ms(k))
            return out

        ys, w = folded()  # warm-up, and a check against the rows
        ys_rows, _ = k.open_device(d_rows, d_zs)
        torch.cuda.synchronize()
        assert torch.equal(ys[0], ys_rows)
        phases.clear()
        ms_f, ms_r = interleaved(folded, lambda: k.open_device(d_rows, d_zs))
        ph = {n: float(np.median([p[n] for p in phases])) for n in pkg.KZG_FOLD_PHASES}
        lines.append("open, K = %2d: open_fold_device %.2f ms (%.2f) with one witness; phases fold %.3f, evals %.3f, quotient %.3f, lincomb %.2f ms; "
                     "open_device on the K polynomials as K rows, K witnesses: %.2f ms (%.2f) = %.2fx the folded call" %
                     (K, np.median(ms_f), min(ms_f), ph["fold"], ph["evals"], ph["quotient"], ph["lincomb"], np.median(ms_r), min(ms_r),
                      np.median(ms_r) / np.median(ms_f)))
    return lines


def step_fold():
    """the fold kernel alone"""
    pkg = cwc_import.load()
    rate = pkg.modmul_rate()
    lines = ["modmul probe: %.3e Fr products per second" % rate]
    d_p = torch.from_numpy(scalars(16 * N, 1).reshape(1, 16, N, 32)).cuda()
    d_g = torch.from_numpy(scalars(1, 3)).cuda()
    pkg.kzg_fold_device(d_p, d_g)
    torch.cuda.synchronize()
    ms, _ = interleaved(lambda: pkg.kzg_fold_device(d_p, d_g), lambda: None)
    read = 16 * N * 32
    lines.append("kzg_fold_device, K = 16: %.3f ms (%.3f) = %.0f GB/s of coefficients read (HBM: 8 000 GB/s); its %d Fr products at the probe's rate: %.3f ms" %
                 (np.median(ms), min(ms), read / np.median(ms) / 1e6, 15 * N, 15 * N / rate * 1e3))
    return lines


def step_verify():
    """verify_fold beside verify on G rows: honest groups of K short polynomials"""
    pkg, k = setup()
    lines = []
    for K in (1, 16, 64):
        short = torch.from_numpy(scalars(K * 64, 5 + K).reshape(1, K, 64, 32)).cuda()
        d_c1 = k.commit_device(short[0].contiguous())
        for G in (1, 1024):
            d_ps = short.expand(G, K, 64, 32).contiguous()
            d_zs, d_gs = torch.from_numpy(scalars(G, 6 + G)).cuda(), torch.from_numpy(scalars(G, 7 + G)).cuda()
            d_ys, d_ws = k.open_fold_device(d_ps, d_zs, d_gs)
            d_cs = d_c1.expand(G, K, 64).contiguous()
            # the single-row side: G honest openings of the first polynomial
            r_ys, r_ws = k.open_device(d_ps[:, 0].contiguous(), d_zs)
            r_cs = d_c1[:1].expand(G, 64).contiguous()
            st = k.verify_fold_device(d_cs, d_zs, d_gs, d_ys, d_ws)
            st_r = k.verify_device(r_cs, d_zs, r_ys, r_ws)
            torch.cuda.synchronize()
            assert not st.cpu().numpy().any() and not st_r.cpu().numpy().any()
            phases = []

            def folded():
                out = k.verify_fold_device(d_cs, d_zs, d_gs, d_ys, d_ws)
                phases.append(pkg.kzg_fold_phase_ms(k))
                return out

            ms_f, ms_r = interleaved(folded, lambda: k.verify_device(r_cs, d_zs, r_ys, r_ws))
            pv = {n: float(np.median([p[n] for p in phases])) for n in pkg.KZG_FOLD_PHASES}
            lines.append("verify, K = %2d, G = %4d: verify_fold_device %.2f ms (%.2f); phases prepare %.2f, pairing and comparison %.2f ms; verify_device on G rows "
                         "%.2f ms (%.2f): the folded call is %+.2f ms" %
                         (K, G, np.median(ms_f), min(ms_f), pv["prepare"], pv["pairing"], np.median(ms_r), min(ms_r), np.median(ms_f) - np.median(ms_r)))
    return lines


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        sys.stdout.write("\n".join({"open": step_open, "fold": step_fold, "verify": step_verify}[sys.argv[2]]()) + "\n")
        return 0
    out = "Folded KZG openings over a power-%d file, polynomials of N = 2^%d coefficients; median of %d (min), HIP events\n" % (POWER, POWER, REPS)
    rc = 0
    for step, limit in STEPS.items():
        if rc != 0:  # nothing more is started on the device after a step that failed
            out += "%s: not measured (an earlier step ended the run)\n" % WHAT[step]
            continue
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            out += "%s: not measured (the step ran past its %d s)\n" % (WHAT[step], limit)
            rc = 124
            continue
        if r.returncode != 0:
            out += "%s: not measured (the step's exit status was %d)\n%s" % (WHAT[step], r.returncode, r.stderr[-2000:])
            rc = r.returncode
            continue
        out += r.stdout
    if rc == 0:
        out += "not measured: G > 1 at N = 2^18 through open_fold; polynomials above 2^18 coefficients; K above 64 in verify_fold\n"
    sys.stdout.write(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out)
    return rc


if __name__ == "__main__":
    sys.exit(main())
