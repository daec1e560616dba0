"""Groth16 key setup of the authV2-class circuit from a powers-of-tau file on the GPU (include/graph_witness_groth16_ptau.h,
gwb_groth16_setup_ptau): the time of the whole call (host clock around the synchronous call) and of its seven device phases
(HIP events) with the Lagrange forms computed and with them read from the file, beside the trapdoor setup's figures from the
same run, and the byte equality of the three keys at (tau, alpha, beta, 1, delta).  The power-18 `.ptau` is made here from a
known tau with the device's generator multiplication (fine for timing; a real file comes from a ceremony).  Of its prepared
sections only the levels the setup reads (p and p + 1) are filled; the others are zero bytes.  The R1CS is the one of
tools/gpu_groth16_setup.py.  Writes the report to stdout and to the path given as the first argument, if any.  A second
argument names a file with the output of
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage -c r1cs/setup_ptau.hip
whose per-kernel register and scratch figures are appended to the report."""
import os
import re
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cwc_import  # noqa: E402
from tests import groth16_fixtures as GF  # noqa: E402
from tests import ptau_fixtures as PF  # noqa: E402
from tests import r1cs_fixtures as F  # noqa: E402

N_PUB = 3
REPS = 3
R = F.R
TAU, ALPHA, BETA, DELTA = 0x1234567 << 200 | 5, 7 << 180 | 11, 13 << 190 | 17, 29 << 210 | 31


def device_points(pkg, group, scalars, chunk=1 << 18):
    """the stored form (affine, Montgomery little-endian) of k G for every k"""
    out = []
    for at in range(0, len(scalars), chunk):
        part = scalars[at:at + chunk]
        arr = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in part), dtype=np.uint8).reshape(len(part), 32)
        raw = pkg.bn254_gen_mul_batch_device(torch.from_numpy(arr.copy()).cuda(), group).cpu().numpy().tobytes()
        out.append(b"".join(GF.lem(int.from_bytes(raw[o:o + 32], "little")) for o in range(0, len(raw), 32)))
    return b"".join(out)


def make_ptau(pkg, power, p):
    points = lambda group, scalars: device_points(pkg, group, scalars)  # noqa: E731
    secs = PF.sections(power, TAU, ALPHA, BETA, points=points)
    n, top = 1 << p, 1 << power
    l1 = PF.lagrange_scalars(p, TAU)

    def levels(group, unit, count, filled):
        body = bytearray(unit * count)
        for m, scalars in filled:
            body[unit * ((1 << m) - 1):unit * ((2 << m) - 1)] = points(group, scalars)
        return bytes(body)

    secs[12] = levels(1, 64, 4 * top - 1, [(p, l1), (p + 1, PF.lagrange_scalars(p + 1, TAU))])
    secs[13] = levels(2, 128, 2 * top - 1, [(p, l1)])
    secs[14] = levels(1, 64, 2 * top - 1, [(p, [ALPHA * x % R for x in l1])])
    secs[15] = levels(1, 64, 2 * top - 1, [(p, [BETA * x % R for x in l1])])
    assert len(l1) == n
    return PF.assemble(secs)


def timed(call, phase_ms, reps):
    walls, phases, out = [], [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        walls.append(time.perf_counter() - t0)
        phases.append(phase_ms())
    return out, walls, {k: float(np.median([ph[k] for ph in phases])) for k in phases[0]}


def resource_lines(path):
    """the compiler's remarks -> one line per kernel"""
    text = open(path).read()
    out = []
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)",
                         text, re.S):
        name = m.group(1)
        kernel = re.search(r"\d+(\w+?_kernel)", name).group(1)
        group = "<G2>" if "Fq2T" in name else "<G1>" if "FqT" in name else ""
        out.append("  %-24s %3s VGPRs, %3s AGPRs, %s bytes of scratch, %s waves / SIMD" % (kernel + group, m.group(2), m.group(3), m.group(4), m.group(5)))
    return out


def main():
    pkg = cwc_import.load()
    C = pkg.graphgen.circuits
    with F.gadget_constraints():
        b = C.build_authv2_class()
    cons = F.derive_r1cs(b)
    r1 = pkg.R1cs(F.write_r1cs(len(b._witness), cons, n_pub_in=N_PUB))
    nv, n, p = r1.info["n_wires"], r1.qap_info()["domain_size"], r1.qap_info()["domain_power"]
    n_terms = r1.info["n_factors_a"] + r1.info["n_factors_b"] + r1.info["n_factors_c"]
    t0 = time.perf_counter()
    ptau = make_ptau(pkg, p + 1, p)
    info = pkg.ptau_info(ptau)
    lines = ["Groth16 key setup from a powers-of-tau file, authV2-class graph (the R1CS of tools/gpu_groth16_setup.py, %d public signals)" % N_PUB,
             "circuit: %d wires, %d constraints, %d terms, domain %d = 2^%d" % (nv, r1.info["n_constraints"], n_terms, n, p),
             "ptau: power %d, %.0f MB, prepared %s, written from a known tau with the device's generator multiplication in %.0f s "
             "(host time, mostly Python integers)" % (info["power"], len(ptau) / 1e6, info["prepared"], time.perf_counter() - t0)]
    keys = {}
    for mode in ("compute", "file"):
        call = lambda: pkg.groth16_setup_ptau(r1, ptau, DELTA, mode)  # noqa: E731
        call()  # warm-up: code objects
        keys[mode], walls, ph = timed(call, pkg.groth16_setup_ptau_phase_ms, REPS)
        lines.append("setup_ptau, lagrange = %s, warm (%d calls): %.0f ms median, %.0f ms min on the host clock" %
                     (mode, REPS, np.median(walls) * 1e3, min(walls) * 1e3))
        lines.append("  device phases (HIP events, median ms): %s; sum %.2f ms" % (", ".join("%s %.2f" % kv for kv in ph.items()), sum(ph.values())))
    trap = (TAU, ALPHA, BETA, 1, DELTA)
    pkg.groth16_setup(r1, trap)
    keys["trapdoor"], walls, ph = timed(lambda: pkg.groth16_setup(r1, trap), pkg.groth16_setup_phase_ms, REPS)
    lines.append("beside it, the trapdoor setup (gwb_groth16_setup) at (tau, alpha, beta, 1, delta) in the same run: %.0f ms median on the host "
                 "clock; device phases %s; sum %.2f ms" % (np.median(walls) * 1e3, ", ".join("%s %.2f" % kv for kv in ph.items()), sum(ph.values())))
    equal = keys["compute"] == keys["file"] == keys["trapdoor"]
    lines.append("the three keys (%.1f MB each) are %s" % (len(keys["trapdoor"]) / 1e6, "byte for byte equal" if equal else "NOT EQUAL"))
    n_mul = (4 * (n // 2) * (p - 1) + n + 4 * n, (n // 2) * (p - 1) + n)
    lines.append("variable-base multiplications of the transforms under compute: %d in G1, %d in G2 (butterflies with k != 0, the odd-half "
                 "pass, the appended 1 / N); delta: %d in G1" % (n_mul[0], n_mul[1], nv - N_PUB - 1 + n))
    lines.append("not measured: snarkjs `zkey new` or `powersoftau prepare phase2` on the same inputs (no snarkjs on the GPU machine)")
    if len(sys.argv) > 2:
        lines.append("registers of r1cs/setup_ptau.hip's kernels (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):")
        lines += resource_lines(sys.argv[2])
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out)
    assert equal
    assert struct.unpack_from("<I", keys["compute"], 4)[0] == 1


if __name__ == "__main__":
    main()
