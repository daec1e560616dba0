"""Diagnostic: where every wave of an interpreter launch sat (gwb_wave_census, diagnostic library) -- waves per SIMD per CU,
and for programs of several streams which roles share a SIMD and how long each role ran.

    python tools/gpu_wave_census.py [key ...]         keys as for set_tile_width (default 0x102 0x902), decimal or 0x..
    PROBE_B=1024 PROBE_GRAPH=authv2|gadgets           batch and graph
    CWC_STREAM_TILES_PER_WORKGROUP=2                  (read by the library) the two-tile workgroup of two-stream divider programs

A wave's record is its HW_ID and XCC_ID registers and s_memtime at its start and end.  A SIMD is (XCC, SE, SH, CU, SIMD); waves
count as sharing one whenever they ran on it during the launch (launches of more waves than the chip holds run in rounds)."""
import collections
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def role_name(r):
    if not r["has_tile"]:
        return "absent"
    return ("div%d" if r["divider"] else "s%d") % r["stream"]


def report(records, out=sys.stdout):
    """records: Graph.wave_census() -> text: waves per SIMD, the roles that share a SIMD, run time per role."""
    simds = collections.defaultdict(list)
    cus = set()
    for r in records:
        cu = (r["xcc"], r["se"], r["sh"], r["cu"])
        cus.add(cu)
        simds[cu + (r["simd"],)].append(r)
    per_simd = collections.Counter(len(v) for v in simds.values())
    print("   waves %d  workgroups %d  CUs used %d  SIMDs used %d; SIMDs holding n waves: %s" % (
        len(records), len({r["workgroup"] for r in records}), len(cus), len(simds),
        ", ".join("%d: %d" % kv for kv in sorted(per_simd.items()))), file=out)
    groups = collections.Counter(" + ".join(sorted(role_name(r) for r in v)) for v in simds.values())
    for names, n in sorted(groups.items(), key=lambda kv: -kv[1]):
        print("   SIMDs holding {%s}: %d" % (names, n), file=out)
    t0 = {}  # (s_memtime is a clock of the XCD: starts are compared within one)
    for r in records:
        t0[r["xcc"]] = min(t0.get(r["xcc"], r["start"]), r["start"])
    by_role = collections.defaultdict(list)
    for r in records:
        if r["end"]:
            by_role[role_name(r)].append((r["start"] - t0[r["xcc"]], r["end"] - r["start"]))
    for name in sorted(by_role):
        st = np.array([a for a, _ in by_role[name]], dtype=np.float64)
        cy = np.array([b for _, b in by_role[name]], dtype=np.float64)
        print("   %-6s waves %5d  start (cycles after its XCD's first) max %.3g  run cycles min %.4g mean %.4g max %.4g" % (
            name, len(cy), st.max(), cy.min(), cy.mean(), cy.max()), file=out)
    alone = [r for v in simds.values() if len(v) == 1 for r in v]
    print("   waves alone on their SIMD: %s" % (dict(collections.Counter(role_name(r) for r in alone)) or "none"), file=out)


def main():
    # the stamped interpreter instances live in the diagnostic library (make diag): loaded in place of the product's
    sys.path.insert(0, ROOT)
    _pkg = os.path.join(ROOT, "circom-witnesscalc_amd")
    if not os.environ.get("CWC_LIB_PATH"):
        diag = os.path.join(_pkg, "libcircom_witnesscalc_amd_diag.so")
        if not os.path.exists(diag):
            subprocess.check_call(["make", "-s", "-C", os.path.join(_pkg, "csrc"), "diag"])
        os.environ["CWC_LIB_PATH"] = diag
    import torch
    import cwc_import
    pkg = cwc_import.load()
    C = pkg.graphgen.circuits
    kind = os.environ.get("PROBE_GRAPH", "authv2")
    g = pkg.Graph((C.build_authv2_class() if kind == "authv2" else C.build_gadgets()).to_bin())
    B = int(os.environ.get("PROBE_B", "1024"))
    rng = np.random.default_rng(1)
    rows = np.frombuffer(rng.bytes(B * g.n_inputs * 32), dtype=np.uint8).reshape(B, g.n_inputs, 32).copy()
    rows[:, :, 31] &= 0x1f
    rows[:, 0, :] = 0
    rows[:, 0, 0] = 1
    d_in = torch.from_numpy(rows).cuda()
    d_out = torch.empty((B, g.n_witness, 32), dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(B, dtype=torch.int32, device="cuda")
    for key in [int(x, 0) for x in sys.argv[1:]] or [0x102, 0x902]:
        g.set_tile_width(key)
        g.calc_witness_batch_device(d_in, d_out, d_st)
        torch.cuda.synchronize()
        t = g.last_timing()
        print("key 0x%x  B=%d  %s  product interp %.2f ms pack %.2f ms  (CWC_STREAM_TILES_PER_WORKGROUP=%s)" % (
            key, B, kind, t["interp_ms"], t["pack_ms"], os.environ.get("CWC_STREAM_TILES_PER_WORKGROUP", "")))
        report(g.wave_census(d_in, d_out, d_st))


if __name__ == "__main__":
    main()
