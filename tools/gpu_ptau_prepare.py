"""Preparing a powers-of-tau file for phase 2 on the GPU, and checking a prepared one (ptau_prepare_phase2, ptau_check_lagrange;
include/graph_witness_groth16_ptau.h), on the power-18 file that tools/gpu_groth16_setup_ptau.py makes on the device and on the
authV2-class R1CS.  Host clock around the synchronous calls, warm, median of 3:
  ptau_prepare_phase2 with its phases, and in the same run the per-level route for the same sections: one
  bn254_point_idft_batch_device call per level (what the all-levels kernel has to beat; the sections go up from host memory and
  the levels come back to it, as in the call itself);
  ptau_check_lagrange for the circuit's domain and for all levels;
  groth16_setup_ptau and groth16_verify_key under compute (what they did before), under file, and under file with
  check_lagrange=True.
Writes the report to stdout and to the path given as the first argument, if any."""
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
TAU, ALPHA, BETA = 0x1234567 << 200 | 5, 7 << 180 | 11, 13 << 190 | 17
SEED = bytes(range(32))
R = GF.R


def device_canonical(pkg, group, scalars, chunk=1 << 18):
    """k G for every k as a device tensor uint8 [n, 64 group], canonical affine"""
    out = []
    for at in range(0, len(scalars), chunk):
        part = scalars[at:at + chunk]
        arr = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in part), dtype=np.uint8).reshape(len(part), 32)
        out.append(pkg.bn254_gen_mul_batch_device(torch.from_numpy(arr.copy()).cuda(), group))
    return torch.cat(out)


def stored(canonical):
    """canonical device points -> the stored form (Montgomery little-endian) as bytes"""
    raw = canonical.cpu().numpy().tobytes()
    return b"".join(GF.lem(int.from_bytes(raw[o:o + 32], "little")) for o in range(0, len(raw), 32))


def walls_of(call, reps=REPS):
    out, walls = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    return out, walls


def main():
    pkg = cwc_import.load()
    C = pkg.graphgen.circuits
    with F.gadget_constraints():
        b = C.build_authv2_class()
    cons = F.derive_r1cs(b)
    r1 = pkg.R1cs(F.write_r1cs(len(b._witness), cons, n_pub_in=N_PUB))
    nv, n, p = r1.info["n_wires"], r1.qap_info()["domain_size"], r1.qap_info()["domain_power"]
    power = p + 1
    lines = ["Preparing a powers-of-tau file for phase 2 and checking it, power %d; authV2-class R1CS (%d wires, domain 2^%d)" % (power, nv, p)]
    t0 = time.perf_counter()
    mono = {}  # the monomial sections as the aid takes them, kept on the device for the per-level route

    def points(group, scalars):
        d = device_canonical(pkg, group, scalars)
        mono[len(mono)] = d
        return stored(d)

    ptau = PF.assemble(PF.sections(power, TAU, ALPHA, BETA, points=points))
    lines.append("the power-%d file (%.0f MB) was made in %.0f s" % (power, len(ptau) / 1e6, time.perf_counter() - t0))
    t1, t2, at, bt = mono[0], mono[1], mono[2], mono[3]

    # -- prepare, and the per-level route
    phases = []

    def prepare():
        out = pkg.ptau_prepare_phase2(ptau)
        phases.append(pkg.ptau_prepare_phase_ms())
        return out

    prepared = prepare()  # code objects
    phases.clear()
    prepared, walls = walls_of(prepare)
    ph = {k: float(np.median([x[k] for x in phases])) for k in phases[0]}
    lines.append("ptau_prepare_phase2, warm (%d calls): %.0f ms median, %.0f ms min on the host clock; output %.0f MB" %
                 (REPS, np.median(walls), min(walls), len(prepared) / 1e6))
    lines.append("  its phases (HIP events, median ms, summed over the four sections): load %.1f, idft_g1 %.1f, idft_g2 %.1f, affine %.1f" %
                 (ph["load"], ph["idft_g1"], ph["idft_g2"], ph["affine"]))
    zero = torch.zeros((1, 64), dtype=torch.uint8, device="cuda")
    hosts = [(torch.cat([t1, zero]).cpu(), 1, power + 1), (t2.cpu(), 2, power), (at.cpu(), 1, power), (bt.cpu(), 1, power)]  # section 12's missing input is O

    def per_level():
        """like for like with the call above: every section goes up from host memory once and every level comes back to it"""
        out = []
        for pts, group, top in hosts:
            d = pts.cuda()
            out.append([d[:1].cpu()] + [pkg.bn254_point_idft_batch_device(d[:1 << m].contiguous(), group).cpu() for m in range(1, top + 1)])
        return out

    per_level()
    _, route = walls_of(per_level)
    lines.append("the per-level route for the same sections (one bn254_point_idft_batch_device call per level, %d calls, each with its own "
                 "load, twiddles and conversion to affine; sections uploaded from and levels copied back to host memory, as the call above "
                 "does; host clock): %.0f ms median, %.0f ms min" % (4 * power + 1, np.median(route), min(route)))
    lines.append("  ptau_prepare_phase2 %s the per-level route (%.0f ms against %.0f ms; the route does not check points or write a file image)" %
                 ("beats" if np.median(walls) < np.median(route) else "DOES NOT beat", np.median(walls), np.median(route)))

    # -- the check
    pkg.ptau_check_lagrange(prepared, p, seed=SEED)
    _, walls = walls_of(lambda: pkg.ptau_check_lagrange(prepared, p))
    lines.append("ptau_check_lagrange for the domain 2^%d, warm (%d calls): %.0f ms median, %.0f ms min on the host clock" % (p, REPS, np.median(walls), min(walls)))
    pkg.ptau_check_lagrange(prepared, seed=SEED)
    _, walls = walls_of(lambda: pkg.ptau_check_lagrange(prepared))
    lines.append("ptau_check_lagrange for all levels, warm (%d calls): %.0f ms median, %.0f ms min on the host clock" % (REPS, np.median(walls), min(walls)))

    # -- the setup and the key check under the three routes
    key = pkg.groth16_setup_ptau(r1, ptau, 1, "compute")
    assert key == pkg.groth16_setup_ptau(r1, prepared, 1, "file")
    medians = {}
    for name, file, kw in (("compute", ptau, {"lagrange": "compute"}), ("file", prepared, {"lagrange": "file"}),
                           ("file, check_lagrange=True", prepared, {"lagrange": "file", "check_lagrange": True})):
        if "check_lagrange" not in kw:
            _, walls = walls_of(lambda: pkg.groth16_setup_ptau(r1, file, 1, kw["lagrange"]))
            lines.append("groth16_setup_ptau(delta = 1), lagrange = %s, warm (%d calls): %.0f ms median" % (name, REPS, np.median(walls)))
        assert pkg.groth16_verify_key(key, r1, file, seed=SEED, **kw) == []
        _, walls = walls_of(lambda: pkg.groth16_verify_key(key, r1, file, **kw))
        medians[name] = float(np.median(walls))
        lines.append("groth16_verify_key (no records), lagrange = %s, warm (%d calls): %.0f ms median" % (name, REPS, medians[name]))
    cheaper = medians["file, check_lagrange=True"] < medians["compute"]
    lines.append("file with the check costs %s than compute (%.0f ms against %.0f ms)" %
                 ("less" if cheaper else "MORE", medians["file, check_lagrange=True"], medians["compute"]))
    lines.append("not measured: snarkjs `powersoftau prepare phase2` on the same file (no snarkjs on the GPU machine); no snarkjs-prepared file was compared")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out)


if __name__ == "__main__":
    main()
