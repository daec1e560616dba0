"""A powers-of-tau contribution and its verification on the GPU (include/graph_witness_groth16_ceremony.h), warm, median of 3:
  the two multiplication aids at 2^18 G1 and 2^17 G2 points with uniform random scalars, `window` against `plain` in interleaved
  rounds of one process (HIP events around each call; the call holds the multiplication kernel and the conversion to affine,
  the same for both methods);
  ptau_contribute on a power-18 file with its five phases (HIP events, summed over the pieces) and the host clock around the call;
  ptau_beacon on that file with its phases (the contribution's path at derived scalars) and the host's hash-chain rate;
  ptau_verify on that file with one and with two records, with the records and without them (the whole-file check alone), host
  clock;
  beside them in the same run groth16_setup_ptau's delta_scale phase on the authV2-class R1CS, the one-scalar reference point
  (scale_points_kernel's wave-uniform scalar over wires - public - 1 + domain G1 points).
The power-18 file has the logs of tools/gpu_groth16_setup_ptau.py; it is made here by ptau_new and one contribution with those
logs, which gives the same sections 1 to 6 (tests/test_gpu_ptau_ceremony.py shows the byte equality at powers 3 and 4).
Writes the report to stdout and to the path given as the first argument, if any.  A second argument names a file with the output of
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage -c r1cs/ceremony.hip
whose per-kernel register, LDS and scratch figures are appended to the report."""
import os
import random
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cwc_import  # noqa: E402
from tests import r1cs_fixtures as F  # noqa: E402

REPS = 3
POWER = 18
N_PUB = 3
R = F.R
TAU, ALPHA, BETA, DELTA = 0x1234567 << 200 | 5, 7 << 180 | 11, 13 << 190 | 17, 29 << 210 | 31
BEACON_HASH, BEACON_EXP = bytes(range(32)), 10


def scalars_device(n, seed):
    rnd = random.Random(seed)
    arr = np.frombuffer(b"".join(rnd.randrange(R).to_bytes(32, "little") for _ in range(n)), dtype=np.uint8).reshape(n, 32)
    return torch.from_numpy(arr.copy()).cuda()


def event_ms(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = call()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def walls_of(call, reps=REPS):
    out, walls = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    return out, walls


def resource_lines(path):
    """the compiler's remarks -> one line per kernel"""
    text = open(path).read()
    out = []
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                         r"LDS Size \[bytes/block\]: (\d+)", text, re.S):
        name = m.group(1)
        kernel = re.search(r"\d+([a-z_]+_kernel)", name).group(1)
        group = "G2" if "Fq2T" in name else "G1" if "FqT" in name else ""
        method = re.search(r"ELj([01])E", name)
        tag = "<%s, %s>" % (group, method.group(1)) if group and method else ""
        out.append("  %-26s %3s VGPRs, %3s AGPRs, %6s bytes of LDS per workgroup, %s bytes of scratch, %s waves / SIMD" %
                   (kernel + tag, m.group(2), m.group(3), m.group(6), m.group(4), m.group(5)))
    return out


def main():
    pkg = cwc_import.load()
    lines = ["A powers-of-tau contribution and its verification, power %d" % POWER]

    # -- the file, and with it the points of the aids' measurement
    t0 = time.perf_counter()
    f0 = pkg.ptau_new(POWER)
    base, _ = pkg.ptau_contribute(f0, secrets=(TAU, ALPHA, BETA))  # also the warm-up: code objects
    lines.append("the power-%d file (%.0f MB) with the logs of tools/gpu_groth16_setup_ptau.py was made by ptau_new and one contribution in %.1f s" %
                 (POWER, len(base) / 1e6, time.perf_counter() - t0))
    n1, n2 = 1 << 18, 1 << 17
    head = 12 + 12 + 44 + 12  # magic, section 1, the header of section 2
    sec2 = np.frombuffer(base, dtype=np.uint8, count=n1 * 64, offset=head).reshape(n1, 64)
    off3 = head + ((2 << POWER) - 1) * 64 + 12
    sec3 = np.frombuffer(base, dtype=np.uint8, count=n2 * 128, offset=off3).reshape(n2, 128)
    aids = {}
    for group, pts, n in ((1, sec2, n1), (2, sec3, n2)):
        d_points, d_scalars = torch.from_numpy(pts.copy()).cuda(), scalars_device(n, 10 + group)
        call = pkg.bn254_g1_mul_batch_device if group == 1 else pkg.bn254_g2_mul_batch_device
        outs, ms = {}, {"window": [], "plain": []}
        for method in ms:  # warm-up
            outs[method] = call(d_points, d_scalars, form="montgomery", method=method)
        torch.cuda.synchronize()
        assert torch.equal(outs["window"], outs["plain"])
        for _ in range(REPS):  # interleaved rounds
            for method in ms:
                ms[method].append(event_ms(lambda: call(d_points, d_scalars, form="montgomery", method=method))[1])
        aids[group] = {k: float(np.median(v)) for k, v in ms.items()}
        lines.append("bn254_g%d_mul_batch_device, %d points of the file, uniform random scalars below r (HIP events, %d interleaved rounds): "
                     "window %.2f ms median (%.2f min), plain %.2f ms median (%.2f min): window is %.2fx plain; the outputs are equal" %
                     (group, n, REPS, aids[group]["window"], min(ms["window"]), aids[group]["plain"], min(ms["plain"]),
                      aids[group]["plain"] / aids[group]["window"]))
    for group in (1, 2):
        lines.append("  G%d: the windowed method is %s than plain in this run" % (group, "FASTER" if aids[group]["window"] < aids[group]["plain"] else "NOT faster"))

    # -- the contribution
    phases = []

    def contribute(image, secrets):
        out = pkg.ptau_contribute(image, secrets=secrets)
        phases.append(pkg.ptau_contribute_phase_ms())
        return out

    (f1, _), walls = walls_of(lambda: contribute(base, (DELTA, ALPHA ^ 5, BETA ^ 9)))
    ph = {k: float(np.median([x[k] for x in phases])) for k in phases[0]}
    lines.append("ptau_contribute, warm (%d calls): %.0f ms median, %.0f ms min on the host clock (%d G1 and %d G2 multiplications, each by its own scalar)" %
                 (REPS, np.median(walls), min(walls), (5 << POWER) - 1, 1 << POWER))
    lines.append("  its phases (HIP events, median ms, summed over the pieces): %s; sum %.1f ms" % (", ".join("%s %.1f" % kv for kv in ph.items()), sum(ph.values())))
    lines.append("  the rest of the call is host work: the file's sections, the record's nine single-point multiplications and three hash_to_g2, the new image")

    # -- the beacon: the contribution's path at derived scalars; the host's hash chain is timed apart at a larger exponent
    phases.clear()

    def beacon(image):
        out = pkg.ptau_beacon(image, BEACON_HASH, BEACON_EXP)
        phases.append(pkg.ptau_contribute_phase_ms())
        return out

    (fb, _), walls_b = walls_of(lambda: beacon(f1))
    pb = {k: float(np.median([x[k] for x in phases])) for k in phases[0]}
    lines.append("ptau_beacon on the file with two records, numIterationsExp %d, warm (%d calls): %.0f ms median, %.0f ms min on the host clock; its "
                 "phases: %s; sum %.1f ms (the contribution's kernels at derived scalars)" %
                 (BEACON_EXP, REPS, np.median(walls_b), min(walls_b), ", ".join("%s %.1f" % kv for kv in pb.items()), sum(pb.values())))
    t0 = time.perf_counter()
    pkg.beacon_scalars(1, BEACON_HASH, 22)
    dt = time.perf_counter() - t0
    lines.append("  the hash chain on this host's CPU: 2^22 links in %.2f s = %.2f million links per second; 2^28 links take %.0f s at that rate" %
                 (dt, (1 << 22) / dt / 1e6, dt * 64))
    assert len(pkg.ptau_verify(fb, require_beacon=True)) == 3
    _, walls_v = walls_of(lambda: pkg.ptau_verify(fb))
    lines.append("ptau_verify of that file (two records and the beacon), warm (%d calls, host clock): %.0f ms median" % (REPS, np.median(walls_v)))

    # -- the verification
    for image, n_rec in ((base, 1), (f1, 2)):
        assert len(pkg.ptau_verify(image)) == n_rec  # warm-up
        _, full = walls_of(lambda: pkg.ptau_verify(image))
        _, whole = walls_of(lambda: pkg.ptau_verify(image, records=False))
        lines.append("ptau_verify with %d record%s, warm (%d calls, host clock): %.0f ms median with the records, %.0f ms median without them (the "
                     "whole-file check alone: host point checks, the subgroup check of section 3, six sums, five pairing equations); the records "
                     "cost the difference, %.0f ms" % (n_rec, "s" if n_rec > 1 else "", REPS, np.median(full), np.median(whole), np.median(full) - np.median(whole)))
    pkg.ptau_verify_step(base, f1)
    _, walls = walls_of(lambda: pkg.ptau_verify_step(base, f1))
    lines.append("ptau_verify_step of the second contribution, warm (%d calls): %.0f ms median on the host clock" % (REPS, np.median(walls)))

    # -- the one-scalar reference point
    C = pkg.graphgen.circuits
    with F.gadget_constraints():
        b = C.build_authv2_class()
    r1 = pkg.R1cs(F.write_r1cs(len(b._witness), F.derive_r1cs(b), n_pub_in=N_PUB))
    nv, n = r1.info["n_wires"], r1.qap_info()["domain_size"]
    assert r1.qap_info()["domain_power"] + 1 == POWER
    pkg.groth16_setup_ptau(r1, base, DELTA, "compute")
    scale = []
    for _ in range(REPS):
        pkg.groth16_setup_ptau(r1, base, DELTA, "compute")
        scale.append(pkg.groth16_setup_ptau_phase_ms()["delta_scale"])
    n_scaled = nv - N_PUB - 1 + n
    lines.append("beside them, groth16_setup_ptau's delta_scale phase on the authV2-class R1CS in the same run (HIP events, median of %d): %.2f ms for "
                 "%d G1 points by ONE wave-uniform scalar = %.3f us per point; the contribution's mul_g1 phase: %.3f us per point with a scalar per point" %
                 (REPS, np.median(scale), n_scaled, np.median(scale) * 1e3 / n_scaled, ph["mul_g1"] * 1e3 / ((5 << POWER) - 1)))
    lines.append("not measured: snarkjs `powersoftau contribute` or `verify` on the same file (no snarkjs on the GPU machine); files above power 18")
    if len(sys.argv) > 2:
        lines.append("registers of r1cs/ceremony.hip's kernels (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):")
        lines += resource_lines(sys.argv[2])
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out)


if __name__ == "__main__":
    main()
