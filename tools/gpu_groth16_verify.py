#!/usr/bin/env python3
"""Groth16 verification throughput on one GPU (include/graph_witness_groth16_verify.h): HIP-event time per call and per proof
of verify_batch_device at batch 1, 64, 1 024 and 16 384 for nPublic 1, 16 and 256 (valid proofs, so every row runs every
phase), pairings per second of the pairing aid, and the Fq products of one verification (counted from the code's schedules)
against the modmul probe's rate.

Proofs are forged through known logs (tests' Key pattern): a handful of distinct valid rows, tiled to the batch size; the
statuses are checked (all VALID) on every measured call.

usage: gpu_groth16_verify.py [--quick]   (--quick: batch 1 and 64 only)
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fq_products():
    """Fq Montgomery products per verified row by phase, from fq12_gfx950.hpp's formulas (nPublic-independent part) and the
    vk_x kernel's Straus loop (per signal and per group of 8)"""
    f2m, f2s = 3, 2
    f6m, f6_01, f6_f2 = 6 * f2m, 5 * f2m, 3 * f2m
    f12m, f12s, csq = 3 * f6m, 2 * f6m, 3 * (f2m + f2m)
    line = 2 * 2 + f6_f2 + 2 * f6_01                      # fq12_mul_line_at
    dbl = 4 * f2m + 6 * f2s                              # g2_dbl_step: mul XY, b' c, a (b - f), b h; six squares
    add = 11 * f2m + 2 * f2s                             # g2_add_step
    n_lines, n_dbl = 102, 64
    miller = n_dbl * f12s + 3 * n_lines * line + n_dbl * dbl + (n_lines - n_dbl) * add + 8
    fq_inv = 254 + 128
    easy = (3 * f2m + 3 * f2s + 3 * f2m + f6m * 2) + f2m * 4 + fq_inv + 3 * f6m + 2 * f12m + 5 * f2m
    n_x_bits, x_ones = 62, bin(4965661367192848881).count("1") - 1
    hard = 3 * (n_x_bits * csq + x_ones * f12m) + 12 * f12m + 4 * csq + 7 * 5 * f2m
    xdbl = 6 * f2m + 3 * f2s                              # xyzz_dbl over Fq2 (U^2, X^2, M^2 squares; six products)
    xadd = 12 * f2m + 2 * f2s
    subgroup = 254 * xdbl + bin(21888242871839275222246405745257275088548364400416034343698204186575808495617).count("1") * xadd
    checks = 8 + 2 * 3 + 2 * 3 * f2m                     # to Montgomery, on-curve tests
    vkx_affine = fq_inv + 4
    return {"miller_loop": miller, "final_exp_easy": easy, "final_exp_hard": hard, "subgroup_B": subgroup,
            "checks_and_vkx_affine": checks + vkx_affine}


def vkx_products(n_public):
    groups = (n_public + 7) // 8
    return groups * 256 * 9 + n_public * 60 * 11  # 4 doublings per window per group; about 60 nonzero 4-bit digits per signal


def main():
    import torch
    import cwc_import
    pkg = cwc_import.load()
    from tests import groth16_fixtures as GF
    from tests.test_gpu_groth16_verify import Key, _proof_rows
    quick = "--quick" in sys.argv
    batches = (1, 64) if quick else (1, 64, 1024, 16384)
    print("device:", torch.cuda.get_device_name(0))
    rate = pkg.modmul_rate()
    print("modmul probe: %.3e Fq-class products/s" % rate)
    fp = fq_products()
    base = sum(fp.values())
    print("Fq products per verified row (counted from the schedules): " + ", ".join("%s %d" % kv for kv in fp.items()) +
          "; total %d + vk_x" % base)
    for n_public in (1, 16, 256):
        key = Key(n_public, 100 + n_public)
        rnd = random.Random(n_public)
        pubs = [[rnd.randrange(GF.R) for _ in range(n_public)] for _ in range(4)]
        rows = _proof_rows(key.forge(pubs))
        pa = pkg._public_array(pubs, 4, n_public)
        for b in batches:
            idx = np.arange(b) % 4
            d_p = torch.from_numpy(np.ascontiguousarray(rows[idx])).cuda()
            d_s = torch.from_numpy(np.ascontiguousarray(pa[idx])).cuda()
            st = key.vk.verify_batch_device(d_p, d_s)  # warm-up (and the key's one-time preparation)
            torch.cuda.synchronize()
            assert not st.cpu().numpy().any(), "a valid row did not verify"
            reps = 5 if b <= 1024 else 2
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                st = key.vk.verify_batch_device(d_p, d_s)
            e1.record()
            torch.cuda.synchronize()
            assert not st.cpu().numpy().any()
            ms = e0.elapsed_time(e1) / reps
            prods = base + vkx_products(n_public)
            print("nPublic %3d  batch %5d: %9.3f ms per call, %8.3f us per proof, %.2e proofs/s; %d Fq products per row -> "
                  "%.2e products/s = %.2f %% of the probe" % (n_public, b, ms, 1e3 * ms / b, b / (ms * 1e-3), prods,
                                                            prods * b / (ms * 1e-3), 100.0 * prods * b / (ms * 1e-3) / rate))
    # the pairing aid
    n = 64 if quick else 4096
    ks = [random.Random(7).randrange(1, GF.R) for _ in range(2)]
    p1, q2 = GF.G1.gen_muls([ks[0]])[0], GF.G2.gen_muls([ks[1]])[0]
    g1 = np.tile(np.frombuffer(GF.proof_bytes(p1, None, None)[:64], np.uint8), (n, 1))
    g2 = np.tile(np.frombuffer(GF.proof_bytes(None, q2, None)[64:192], np.uint8), (n, 1))
    d1, d2 = torch.from_numpy(g1).cuda(), torch.from_numpy(g2).cuda()
    out = pkg.bn254_pairing_batch_device(d1, d2)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        out = pkg.bn254_pairing_batch_device(d1, d2)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 3
    assert (out.cpu().numpy() == out.cpu().numpy()[0]).all()
    print("pairing aid: %d pairs in %.3f ms per call = %.3e pairings/s" % (n, ms, n / (ms * 1e-3)))


if __name__ == "__main__":
    main()
