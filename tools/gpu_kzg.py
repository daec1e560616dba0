"""KZG commitments over a powers-of-tau file on the GPU (include/graph_witness_kzg.h), one MI355X, warm, median of 3, HIP events
for the device phases and the host clock for the calls, on a power-18 file that the device makes (ptau_new and one contribution):
  the evaluate-and-quotient kernels at N = 2^18 for every tile of kzg_tiles(), at K = 1 and K = 16 pairs, beside the time the
  modmul probe's rate gives for the same number of Fr products (2 per coefficient and level);
  commit and open at N = 2^18 with open's phases, beside the bn254_g1_lincomb_device aid on the same points and scalars: the
  time of the dominant phase before this layer existed;
  verify at 1, 1 024 and 16 384 openings with its phases, beside bn254_pairing_batch_device for twice that many pairings.
Writes the report to stdout and to the path given as the first argument, if any."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cwc_import  # noqa: E402

REPS = 3
POWER = 18
N = 1 << POWER
TAU, ALPHA, BETA = 0x1234567 << 200 | 5, 7 << 180 | 11, 13 << 190 | 17


def scalars(n, seed):
    """uint8 [n, 32]: uniform values below 2^253 (all below r)"""
    arr = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
    arr[:, 31] &= 0x1f
    return arr


def event_ms(call, reps=REPS):
    """(the last result, [ms]) of `reps` calls, each between two events on the current stream"""
    out, ms = None, []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return out, ms


def walls_of(call, reps=REPS):
    out, walls = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    return out, walls


def levels(n, tile):
    k = 1
    while n > tile:
        n, k = -(-n // tile), k + 1
    return k


def main():
    pkg = cwc_import.load()
    lines = ["KZG commitments over a power-%d file, polynomials of N = 2^%d coefficients" % (POWER, POWER)]
    t0 = time.perf_counter()
    ptau, _ = pkg.ptau_contribute(pkg.ptau_new(POWER), secrets=(TAU, ALPHA, BETA))
    t1 = time.perf_counter()
    k = pkg.Kzg(ptau)
    lines.append("the file (%.0f MB) was made by ptau_new and one contribution in %.1f s; the handle over its %d points (host checks, canonical form) in %.1f s" %
                 (len(ptau) / 1e6, t1 - t0, k.info["max_len"], time.perf_counter() - t1))
    rate = pkg.modmul_rate()
    lines.append("modmul probe: %.3e Fr products per second" % rate)

    # -- the evaluate-and-quotient kernels
    polys16 = torch.from_numpy(scalars(16 * N, 1).reshape(16, N, 32)).cuda()
    zs16 = torch.from_numpy(scalars(16, 2)).cuda()
    ref = None
    for tile in pkg.kzg_tiles():
        for pairs in (1, 16):
            d_p, d_z = polys16[:pairs].contiguous(), zs16[:pairs].contiguous()
            out = pkg.kzg_eval_quotient_device(d_p, d_z, tile=tile)  # warm-up
            torch.cuda.synchronize()
            if pairs == 16:
                if ref is None:
                    ref = out
                else:
                    assert torch.equal(ref[0], out[0]) and torch.equal(ref[1], out[1])
            _, ms = event_ms(lambda: pkg.kzg_eval_quotient_device(d_p, d_z, tile=tile))
            products = 2 * N * pairs * levels(N, tile)
            bytes_moved = pairs * N * 32 * 3  # the coefficients twice (totals, apply), the quotient once
            lines.append("evaluate-and-quotient, tile %4d, K = %2d (%d levels): %.3f ms median (%.3f min) = %.2f ns per coefficient, %.0f GB/s of coefficients "
                         "and quotients; %d Fr products at the probe's rate: %.3f ms" %
                         (tile, pairs, levels(N, tile), np.median(ms), min(ms), np.median(ms) * 1e6 / (N * pairs), bytes_moved / np.median(ms) / 1e6, products,
                          products / rate * 1e3))
    lines.append("  the tiles give equal bytes at K = 16")

    # -- commit and open
    poly, z = polys16[:1].cpu().numpy(), zs16[:1].cpu().numpy()
    d_poly, d_z = polys16[:1].contiguous(), zs16[:1].contiguous()
    head = 12 + 12 + 44 + 12  # magic, section 1, the header of section 2
    sec2 = torch.from_numpy(np.frombuffer(ptau, dtype=np.uint8, count=N * 64, offset=head).reshape(N, 64).copy()).cuda()
    aid = pkg.bn254_g1_lincomb_device(sec2, d_poly[0].contiguous(), form="montgomery")
    torch.cuda.synchronize()
    _, ms_aid = event_ms(lambda: pkg.bn254_g1_lincomb_device(sec2, d_poly[0].contiguous(), form="montgomery"))
    lines.append("bn254_g1_lincomb_device over the file's first 2^%d points with the polynomial's coefficients (the existing aid): %.2f ms median (%.2f min)" %
                 (POWER, np.median(ms_aid), min(ms_aid)))
    c = k.commit_device(d_poly)
    torch.cuda.synchronize()
    _, ms_c = event_ms(lambda: k.commit_device(d_poly))
    _, walls_c = walls_of(lambda: k.commit(poly))
    lines.append("commit, K = 1: commit_device %.2f ms median (%.2f min) by HIP events = %.2fx the aid; commit from host arrays %.1f ms median on the host clock" %
                 (np.median(ms_c), min(ms_c), np.median(ms_c) / np.median(ms_aid), np.median(walls_c)))
    del aid
    phases = []

    def open_once():
        out = k.open_device(d_poly, d_z)
        phases.append(pkg.kzg_phase_ms(k))
        return out

    ys, ws = open_once()
    phases.clear()
    _, ms_o = event_ms(open_once)
    ph = {n: float(np.median([p[n] for p in phases])) for n in phases[0]}
    _, walls_o = walls_of(lambda: k.open(poly, z))
    lines.append("open, K = 1: open_device %.2f ms median (%.2f min); phases quotient %.3f ms, lincomb %.2f ms: the witness's linear combination is %.1f %% of "
                 "the call; open from host arrays %.1f ms median on the host clock" %
                 (np.median(ms_o), min(ms_o), ph["quotient"], ph["lincomb"], 100 * ph["lincomb"] / (ph["quotient"] + ph["lincomb"]), np.median(walls_o)))
    st = k.verify_device(c, d_z, ys, ws)
    assert list(st.cpu().numpy()) == [pkg.KZG_VALID]

    # -- verify: honest openings of one short polynomial at many points
    short = torch.from_numpy(scalars(64, 5).reshape(1, 64, 32)).cuda()
    for count in (1, 1024, 16384):
        d_ps = short.expand(count, 64, 32).contiguous()
        d_zs = torch.from_numpy(scalars(count, 6 + count)).cuda()
        d_ys, d_ws = k.open_device(d_ps, d_zs)
        d_cs = k.commit_device(short).expand(count, 64).contiguous()
        st = k.verify_device(d_cs, d_zs, d_ys, d_ws)
        torch.cuda.synchronize()
        assert not st.cpu().numpy().any()
        phases.clear()

        def verify_once():
            out = k.verify_device(d_cs, d_zs, d_ys, d_ws)
            phases.append(pkg.kzg_phase_ms(k))
            return out

        _, ms_v = event_ms(verify_once)
        pv = {n: float(np.median([p[n] for p in phases])) for n in phases[0]}
        g1 = torch.cat([d_cs, d_ws]).contiguous()
        g2 = torch.from_numpy(np.tile(np.frombuffer(gen2_bytes(), dtype=np.uint8), (2 * count, 1)).copy()).cuda()
        pkg.bn254_pairing_batch_device(g1, g2)
        torch.cuda.synchronize()
        _, ms_p = event_ms(lambda: pkg.bn254_pairing_batch_device(g1, g2))
        lines.append("verify, %5d openings: %.2f ms median (%.2f min) = %.1f us per opening; phases prepare %.2f ms, pairing and comparison %.2f ms; "
                     "bn254_pairing_batch_device for %d pairings: %.2f ms median = %.2fx" %
                     (count, np.median(ms_v), min(ms_v), np.median(ms_v) * 1e3 / count, pv["prepare"], pv["pairing"], 2 * count, np.median(ms_p),
                      np.median(ms_v) / np.median(ms_p)))
    lines.append("not measured: polynomials above 2^18 coefficients; a batch of 2^18-coefficient openings (K > 1 through open); commit_evals")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out)


def gen2_bytes():
    """the G2 generator, canonical"""
    from tests import groth16_fixtures as GF
    (x0, x1), (y0, y1) = GF.G2_GEN
    return b"".join(v.to_bytes(32, "little") for v in (x0, x1, y0, y1))


if __name__ == "__main__":
    main()
