"""The key check on the authV2-class key on the GPU (groth16_verify_key, include/graph_witness_groth16_contribute.h): the time of
a check of the key with two contributions against its circuit and its powers-of-tau file (host clock around the synchronous
call), split into the remake of the key with delta = 1, the linear combinations over C and H and the batched pairings (the
library's own host clock around its three synchronous parts); of ptau_check_powers for the circuit's domain, with its G1 and
G2 linear combinations measured beside it through the aids; and, in the same run, of groth16_setup_ptau itself, which the remake
is.  The power-18 `.ptau` is made here from a known tau with the device's generator multiplication, the key from it with
delta = 1 and two contributions.  The R1CS is the one of tools/gpu_groth16_setup.py.  Writes the report to stdout and to the path
given as the first argument, if any."""
import os
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
TAU, ALPHA, BETA, D1, D2 = 0x1234567 << 200 | 5, 7 << 180 | 11, 13 << 190 | 17, 29 << 210 | 31, 37 << 205 | 41
SEED = bytes(range(32))


def device_points(pkg, group, scalars, chunk=1 << 18):
    """the stored form (affine, Montgomery little-endian) of k G for every k"""
    out = []
    for at in range(0, len(scalars), chunk):
        part = scalars[at:at + chunk]
        arr = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in part), dtype=np.uint8).reshape(len(part), 32)
        raw = pkg.bn254_gen_mul_batch_device(torch.from_numpy(arr.copy()).cuda(), group).cpu().numpy().tobytes()
        out.append(b"".join(GF.lem(int.from_bytes(raw[o:o + 32], "little")) for o in range(0, len(raw), 32)))
    return b"".join(out)


def section_offset(zkey, want):
    """where the body of section `want` starts in a `.zkey`"""
    off = 12
    for _ in range(struct.unpack_from("<I", zkey, 8)[0]):
        sid, size = struct.unpack_from("<IQ", zkey, off)
        if sid == want:
            return off + 12
        off += 12 + size
    raise ValueError("no section %d" % want)


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
    lines = ["Groth16 key check, authV2-class key (the R1CS of tools/gpu_groth16_setup.py, %d public signals)" % N_PUB,
             "circuit: %d wires, domain %d = 2^%d; sections 8 and 9 hold %d points" % (nv, n, p, n_pts)]
    t0 = time.perf_counter()
    ptau = PF.assemble(PF.sections(p + 1, TAU, ALPHA, BETA, points=lambda group, scalars: device_points(pkg, group, scalars)))
    lines.append("the power-%d file (%.0f MB) was made in %.0f s" % (p + 1, len(ptau) / 1e6, time.perf_counter() - t0))

    setup_phases = []

    def setup():
        out = pkg.groth16_setup_ptau(r1, ptau, 1, "compute")
        setup_phases.append(sum(pkg.groth16_setup_ptau_phase_ms().values()))
        return out

    setup()  # code objects
    key0, setup_walls = walls_of(setup)
    key1, h1 = pkg.groth16_contribute(key0, name="first", delta=D1)
    key2, h2 = pkg.groth16_contribute(key1, name="second", delta=D2)
    lines.append("key: %.1f MB, groth16_setup_ptau(delta = 1, compute) and two contributions" % (len(key2) / 1e6))

    assert pkg.groth16_verify_key(key2, r1, ptau, seed=SEED) == [h1, h2]  # warm-up
    phases = []

    def check():
        out = pkg.groth16_verify_key(key2, r1, ptau)
        phases.append(pkg.groth16_verify_key_phase_ms())
        return out

    hashes, walls = walls_of(check)
    ph = {k: float(np.median([x[k] for x in phases])) for k in phases[0]}
    lines.append("groth16_verify_key, lagrange = compute, 2 records, warm (%d calls): %.0f ms median, %.0f ms min on the host clock (key and file "
                 "parsed and checked on the host, the remake, section 4 compared with the circuit, BLAKE2b of the remade key and of rho, "
                 "4 linear combinations, 16 pairings)" % (REPS, np.median(walls), min(walls)))
    lines.append("  its parts (the library's host clock, median ms): remake %.0f, linear combinations %.1f, pairings %.1f; the rest, %.0f ms, is "
                 "host work" % (ph["remake"], ph["lincomb"], ph["pairings"], np.median(walls) - sum(ph.values())))
    _, walls = walls_of(lambda: pkg.groth16_verify_key(key2, r1, ptau, records=False))
    lines.append("  records=False: %.0f ms median" % np.median(walls))
    lines.append("beside it, in the same run: groth16_setup_ptau(delta = 1, compute), warm (%d calls): %.0f ms median on the host clock, %.0f ms "
                 "in its device phases" % (REPS, np.median(setup_walls), np.median(setup_phases[1:])))

    pkg.ptau_check_powers(ptau, p, seed=SEED)
    _, walls = walls_of(lambda: pkg.ptau_check_powers(ptau, p))
    lines.append("ptau_check_powers for the domain 2^%d, warm (%d calls): %.0f ms median, %.0f ms min on the host clock (the %d points read are "
                 "checked on the host first, then the subgroup check of %d G2 points, the five sums in G1 and the one in G2, 10 pairings)" %
                 (p, REPS, np.median(walls), min(walls), 4 * n + n, n + 1))
    rho = torch.randint(0, 256, (2 * n, 16), dtype=torch.uint8, device="cuda")
    pts1 = pkg.bn254_gen_mul_batch_device(torch.randint(0, 256, (2 * n, 32), dtype=torch.uint8, device="cuda"), 1)
    pts2 = pkg.bn254_gen_mul_batch_device(torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda"), 2)
    lines.append("  its device work measured through the aids: one G1 linear combination of %d points %.2f ms, one G2 linear combination of %d "
                 "points %.2f ms" % (2 * n, events_ms(lambda: pkg.bn254_g1_lincomb128_device(pts1, rho)), n,
                                     events_ms(lambda: pkg.bn254_g2_lincomb128_device(pts2, rho[:n].contiguous()))))
    _, walls = walls_of(lambda: pkg.groth16_verify_key(key2, r1, ptau, check_ptau=True))
    lines.append("groth16_verify_key with check_ptau=True: %.0f ms median" % np.median(walls))
    bad = bytearray(key2)
    at = section_offset(key2, 9) + 64 * 5
    bad[at:at + 64] = GF.g1_bytes(GF.G1_GEN)
    try:
        pkg.groth16_verify_key(bytes(bad), r1, ptau)
        refusal = "ACCEPTED"
    except pkg.WitnessCalcError as e:
        refusal = str(e)
    lines.append("one point of H replaced: %s" % refusal)
    lines.append("not measured: `snarkjs zkey verify` on the same key (no snarkjs on the GPU machine)")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out)
    assert hashes == [h1, h2] and refusal.startswith("zkey verify: section 9 (H)")


if __name__ == "__main__":
    main()
