#!/usr/bin/env python3
"""Cost of the compressed point form on one GPU (include/graph_witness_groth16_compressed.h, r1cs/codec.hip), warm, median of 3,
HIP events:

  * the four point kernels at 2^16 points per group (compress and decompress, G1 and G2, canonical form);
  * verify_batch_compressed_device against verify_batch_device on the same 16 384 proofs (nPublic 1, valid proofs forged through
    known logs as in tools/gpu_groth16_verify.py), interleaved in one process;
  * prove_batch_compressed_device against prove_batch_device at 64 rows of the authV2-class key (tools/gpu_groth16.py's system).

By operation count a proof's three roots are about 2 000 Fq products (G1: 252 squarings and about 125 products each; G2: two such
exponentiations and an inversion of 254 + 128) against about 41 000 for its verification, roughly 5 %.  The report says what was
measured beside that.  Writes the report to stdout and to the path given as the first argument, if any.

usage: gpu_groth16_compressed.py [OUT] [--quick]   (--quick: 2^10 points, 256 proofs, no prover part)
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps=3):
    """median and minimum ms of `reps` calls, each between two HIP events, after one warm-up call"""
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    import torch
    import cwc_import
    pkg = cwc_import.load()
    from tests import groth16_fixtures as GF
    from tests import point_codec_cases as PC
    from tests.test_gpu_groth16_verify import Key, _proof_rows
    quick = "--quick" in sys.argv
    out_path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    lines = ["Compressed BN254 points, Groth16 proofs and keys on one MI355X (tools/gpu_groth16_compressed.py; HIP-event time per call, "
             "median of 3 after a warm-up call, min in brackets)", "device: %s" % torch.cuda.get_device_name(0)]
    rate = pkg.modmul_rate()
    lines.append("modmul probe: %.3e Fq-class products/s" % rate)
    sqrt_products = 252 + bin(PC.SQRT_EXP).count("1")
    inv_products = 254 + bin(PC.Q - 2).count("1")
    root_g1, root_g2 = sqrt_products + 6, 2 * sqrt_products + inv_products + 20
    lines.append("Fq products per decoded point (counted from point_codec_gfx950.hpp): G1 %d, G2 %d; per proof %d" %
                 (root_g1, root_g2, 2 * root_g1 + root_g2))

    # -- the point kernels ---------------------------------------------------------------------------------------------------------
    n = 1 << (10 if quick else 16)
    for group, name in ((1, "G1"), (2, "G2")):
        pts = PC.sample_points(group, 64)
        raw = b"".join((PC.g1_bytes if group == 1 else PC.g2_bytes)(p) for p in pts)
        host = np.frombuffer(raw, np.uint8).reshape(64, 64 * group)
        d_pts = torch.from_numpy(np.ascontiguousarray(host[np.arange(n) % 64])).cuda()
        comp = pkg.bn254_g1_compress_batch_device if group == 1 else pkg.bn254_g2_compress_batch_device
        dec = pkg.bn254_g1_decompress_batch_device if group == 1 else pkg.bn254_g2_decompress_batch_device
        d_c = comp(d_pts)
        back, st = dec(d_c)
        torch.cuda.synchronize()
        assert torch.equal(back, d_pts) and not st.any()
        for what, fn, prods in (("compress", lambda: comp(d_pts), 0), ("decompress", lambda: dec(d_c), root_g1 if group == 1 else root_g2)):
            med, lo = timed(fn)
            tail = "; %.2e Fq products/s = %.1f %% of the probe" % (prods * n / (med * 1e-3), 100.0 * prods * n / (med * 1e-3) / rate) if prods else ""
            lines.append("%s %-10s %6d points: %8.3f ms [%.3f], %7.2f ns per point, %.2e points/s%s" %
                         (name, what, n, med, lo, 1e6 * med / n, n / (med * 1e-3), tail))

    # -- the verifier ----------------------------------------------------------------------------------------------------------------
    b = 256 if quick else 16384
    key = Key(1, 101)
    rnd = random.Random(1)
    pubs = [[rnd.randrange(GF.R)] for _ in range(4)]
    rows = _proof_rows(key.forge(pubs))
    pa = pkg._public_array(pubs, 4, 1)
    idx = np.arange(b) % 4
    d_p = torch.from_numpy(np.ascontiguousarray(rows[idx])).cuda()
    d_s = torch.from_numpy(np.ascontiguousarray(pa[idx])).cuda()
    d_cp = pkg.groth16_compress_proofs_device(d_p)
    torch.cuda.synchronize()
    raw_ms, comp_ms, dec_ms = [], [], []
    for fn in (lambda: key.vk.verify_batch_device(d_p, d_s), lambda: key.vk.verify_batch_compressed_device(d_cp, d_s)):   # warm-up
        assert not fn().cpu().numpy().any(), "a valid row did not verify"
    for _ in range(3):   # interleaved: raw, compressed, the decoding alone
        for fn, acc in ((lambda: key.vk.verify_batch_device(d_p, d_s), raw_ms), (lambda: key.vk.verify_batch_compressed_device(d_cp, d_s), comp_ms),
                        (lambda: pkg.groth16_decompress_proofs_device(d_cp), dec_ms)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1))
    r, c, d = (float(np.median(x)) for x in (raw_ms, comp_ms, dec_ms))
    lines.append("verify, nPublic 1, %d proofs: raw %.3f ms [%.3f] (%.3f us per proof), compressed %.3f ms [%.3f] (%.3f us per proof): "
                 "ratio %.4f; decompress_proofs alone %.3f ms [%.3f] = %.2f %% of the raw call" %
                 (b, r, min(raw_ms), 1e3 * r / b, c, min(comp_ms), 1e3 * c / b, c / r, d, min(dec_ms), 100.0 * d / r))
    lines.append("by operation count: %d Fq products per proof to decode against about 41 108 to verify = %.1f %%" %
                 (2 * root_g1 + root_g2, 100.0 * (2 * root_g1 + root_g2) / 41108))

    # -- the prover ------------------------------------------------------------------------------------------------------------------
    if not quick:
        from tests import r1cs_fixtures as F
        from tools.synth import synth_inputs
        C = pkg.graphgen.circuits
        with F.gadget_constraints():
            bld = C.build_authv2_class()
        cons = F.derive_r1cs(bld)
        g = pkg.Graph(bld.to_bin())
        r1 = pkg.R1cs(F.write_r1cs(len(bld._witness), cons))
        K = GF.KnownLog(r1.info["n_wires"], 0, r1.qap_info()["domain_size"])
        pr = pkg.Groth16(K.zkey, r1)
        batch = 64
        d_in = torch.from_numpy(synth_inputs("field", g.n_inputs, batch, 41)).cuda()
        d_w = torch.empty((batch, g.n_witness, 32), dtype=torch.uint8, device="cuda")
        d_st = torch.zeros(batch, dtype=torch.int32, device="cuda")
        g.calc_witness_batch_device(d_in, d_w, d_st)
        torch.cuda.synchronize()
        assert not d_st.cpu().numpy().any()
        rs = [(1 + i, 2 + i) for i in range(batch)]
        p_raw = pr.prove_batch_device(d_w, rs=rs)
        p_c = pr.prove_batch_compressed_device(d_w, rs=rs)
        torch.cuda.synchronize()
        assert torch.equal(pkg.groth16_decompress_proofs_device(p_c)[0], p_raw)
        raw_ms, comp_ms = [], []
        for _ in range(3):
            for fn, acc in ((lambda: pr.prove_batch_device(d_w, rs=rs), raw_ms), (lambda: pr.prove_batch_compressed_device(d_w, rs=rs), comp_ms)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                acc.append(e0.elapsed_time(e1))
        r, c = float(np.median(raw_ms)), float(np.median(comp_ms))
        lines.append("prove, authV2-class key, %d rows: raw %.2f ms [%.2f], compressed %.2f ms [%.2f]: ratio %.4f" %
                     (batch, r, min(raw_ms), c, min(comp_ms), c / r))
    lines.append("not measured: arkworks itself (none is installed here; parity rests on the restated format and its anchors)")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if out_path:
        open(out_path, "w").write(out)


if __name__ == "__main__":
    main()
