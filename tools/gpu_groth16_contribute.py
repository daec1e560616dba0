"""Groth16 phase-2 contributions on the authV2-class key on the GPU (include/graph_witness_groth16_contribute.h): the time of a
contribution (host clock around the synchronous call) and of its three device phases (HIP events, summed over the pieces); of
a step check, with the time of its two kinds of device work measured beside it through the aids (the linear combination of
as many points as sections 8 and 9 hold, and a batch of as many pairings as the check makes); of groth16_verify_contributions
for 1 and 8 records; and, in the same run, the delta_scale phase of groth16_setup_ptau, which multiplies the same number of
points by one scalar.  The key with delta = 1 comes from the trapdoor setup at (tau, alpha, beta, 1, 1), byte for byte the key
of groth16_setup_ptau(delta=1) for a file of those logs; the power-18 `.ptau` for the delta_scale figure is made here from a
known tau with the device's generator multiplication.  The R1CS is the one of tools/gpu_groth16_setup.py.  Writes the report to
stdout and to the path given as the first argument, if any."""
import os
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


def walls_of(call, reps=REPS):
    out, walls = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    return out, walls


def events_ms(call, reps=REPS):
    """median device time of an asynchronous call between two events on the current stream"""
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    pkg = cwc_import.load()
    C = pkg.graphgen.circuits
    with F.gadget_constraints():
        b = C.build_authv2_class()
    cons = F.derive_r1cs(b)
    r1 = pkg.R1cs(F.write_r1cs(len(b._witness), cons, n_pub_in=N_PUB))
    nv, n, p = r1.info["n_wires"], r1.qap_info()["domain_size"], r1.qap_info()["domain_power"]
    n_pts = nv - N_PUB - 1 + n
    lines = ["Groth16 phase-2 contributions, authV2-class key (the R1CS of tools/gpu_groth16_setup.py, %d public signals)" % N_PUB,
             "circuit: %d wires, domain %d = 2^%d; sections 8 and 9 hold %d points" % (nv, n, p, n_pts)]
    key0 = pkg.groth16_setup(r1, (TAU, ALPHA, BETA, 1, 1))
    lines.append("key with delta = 1: %.1f MB, from the trapdoor setup at (tau, alpha, beta, 1, 1)" % (len(key0) / 1e6))

    pkg.groth16_contribute(key0, name="warm-up", delta=DELTA)  # code objects
    phases = []

    def one():
        out = pkg.groth16_contribute(key0, name="first", delta=DELTA)
        phases.append(pkg.groth16_contribute_phase_ms())
        return out

    (key1, _), walls = walls_of(one)
    ph = {k: float(np.median([x[k] for x in phases])) for k in phases[0]}
    lines.append("contribution, warm (%d calls): %.0f ms median, %.0f ms min on the host clock (parsing and checking the key on the host, "
                 "five single-point multiplications on the host, the device phases, the file)" % (REPS, np.median(walls), min(walls)))
    lines.append("  device phases (HIP events, median ms): %s; sum %.2f ms" % (", ".join("%s %.2f" % kv for kv in ph.items()), sum(ph.values())))
    trap = pkg.groth16_setup(r1, (TAU, ALPHA, BETA, 1, DELTA))
    same = key1[:len(trap) - 80] == trap[:len(trap) - 80]  # up to the header of section 10
    lines.append("sections 1 to 9 of the contributed key are %s those of the trapdoor setup at delta" % ("byte for byte" if same else "NOT"))

    # the beacon: the contribution's path at a derived secret (include/graph_witness_groth16_beacon.h)
    phases.clear()

    def beacon():
        out = pkg.groth16_beacon(key1, bytes(range(32)), 10, name="beacon")
        phases.append(pkg.groth16_contribute_phase_ms())
        return out

    (key_b, _), walls_b = walls_of(beacon)
    pb = {k: float(np.median([x[k] for x in phases])) for k in phases[0]}
    assert len(pkg.groth16_verify_contributions(key_b, require_beacon=True)) == 2
    lines.append("beacon on top of it, numIterationsExp 10, warm (%d calls): %.0f ms median, %.0f ms min on the host clock; device phases: %s; sum "
                 "%.2f ms (the contribution's kernels at a derived secret)" %
                 (REPS, np.median(walls_b), min(walls_b), ", ".join("%s %.2f" % kv for kv in pb.items()), sum(pb.values())))

    pkg.groth16_verify_contribution_step(key0, key1)
    _, walls = walls_of(lambda: pkg.groth16_verify_contribution_step(key0, key1))
    lines.append("step check key0 -> key1, warm (%d calls): %.0f ms median, %.0f ms min on the host clock (both keys parsed and checked on "
                 "the host, rho from BLAKE2b on the host, 4 linear combinations, 8 pairings)" % (REPS, np.median(walls), min(walls)))
    pts = pkg.bn254_gen_mul_batch_device(torch.randint(0, 256, (n_pts, 32), dtype=torch.uint8, device="cuda"), 1)
    rho = torch.randint(0, 256, (n_pts, 16), dtype=torch.uint8, device="cuda")
    lines.append("  its device work measured through the aids: one linear combination of %d points %.2f ms (the check makes two per piece, "
                 "in one launch); a batch of 8 pairings %.2f ms" %
                 (n_pts, events_ms(lambda: pkg.bn254_g1_lincomb128_device(pts, rho)),
                  events_ms(lambda: pkg.bn254_pairing_batch_device(pts[:8].contiguous(), pkg.bn254_gen_mul_batch_device(rho[:8].repeat(1, 2).contiguous(), 2)))))
    lines.append("  the scale aid on %d points: %.2f ms (the contribution's kernel and the conversion to affine)" %
                 (n_pts, events_ms(lambda: pkg.bn254_g1_scale_batch_device(pts, DELTA))))

    keys = [key1]
    for k in range(7):
        keys.append(pkg.groth16_contribute(keys[-1], name="party %d" % (k + 2))[0])
    for count in (1, 8):
        key = keys[count - 1]
        assert len(pkg.groth16_verify_contributions(key)) == count
        _, walls = walls_of(lambda: pkg.groth16_verify_contributions(key))
        lines.append("groth16_verify_contributions, %d record%s, warm (%d calls): %.0f ms median on the host clock (%d pairings in one launch)" %
                     (count, "" if count == 1 else "s", REPS, np.median(walls), 8 * count + 4))

    t0 = time.perf_counter()
    ptau = PF.assemble(PF.sections(p + 1, TAU, ALPHA, BETA, points=lambda group, scalars: device_points(pkg, group, scalars)))
    made = time.perf_counter() - t0
    pkg.groth16_setup_ptau(r1, ptau, DELTA, "compute")
    ds = []
    for _ in range(REPS):
        from_ptau = pkg.groth16_setup_ptau(r1, ptau, DELTA, "compute")
        ds.append(pkg.groth16_setup_ptau_phase_ms()["delta_scale"])
    lines.append("beside it, in the same run: the delta_scale phase of groth16_setup_ptau (%d points already on the device in XYZZ form, one "
                 "scalar, plus two single points): %.2f ms median of %d calls (the power-%d file was made in %.0f s)" %
                 (n_pts, float(np.median(ds)), REPS, p + 1, made))
    lines.append("the key of groth16_setup_ptau at delta is %s the trapdoor setup's" % ("byte for byte" if from_ptau == trap else "NOT"))
    lines.append("not measured: snarkjs `zkey contribute` or `zkey verify` on the same key (no snarkjs on the GPU machine)")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out)
    assert same and from_ptau == trap


if __name__ == "__main__":
    main()
