"""What the pack schedule (csrc/pack_schedule.cc) makes of a graph at a batch size, on the host: requests, rows ready at some
request, rows produced behind the last one, and the divider waves' share (n_inline).  No device is touched.

    python tools/pack_schedule_report.py                       # the authV2-class graph at 1024 and 2048 sets
    python tools/pack_schedule_report.py --graph path/to/graph.bin --batch 1024 --key 0x102
    CWC_PACK_PASS_CYCLES=3000 python tools/pack_schedule_report.py    # what-if: another cost of a pack pass
"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import cwc_import
pkg = cwc_import.load()
import program_emulator as pe

C_DIVREQ = 9
ap = argparse.ArgumentParser()
ap.add_argument("--graph", default=None, help="a .bin graph (default: the generated authV2-class graph)")
ap.add_argument("--batch", type=int, action="append", help="batch sizes (default 1024 and 2048)")
ap.add_argument("--key", type=lambda s: int(s, 0), default=0, help="program key (default: the cost model's choice for the batch)")
a = ap.parse_args()
data = open(a.graph, "rb").read() if a.graph else pkg.graphgen.circuits.build_authv2_class().to_bin()
g = pkg.Graph(data)
for batch in a.batch or [1024, 2048]:
    key = a.key or g.pick_tile_width(batch)
    blob = pe.Blob(g.export_blob(key))
    order, ready, n_inline = g.pack_schedule(key)
    req = np.nonzero((np.asarray(blob.hdr, dtype=np.uint64) & np.uint64(15)) == C_DIVREQ)[0]
    nw = order.size
    consts = int(ready[0]) if ready.size else 0
    print("batch %d: program key %#x (T = %d, divider %d, streams %d): %d bundles, %d requests%s" % (
        batch, key, blob.T, blob.divider, blob.n_streams, blob.n_bundles, len(req), ", the last at bundle %d" % req[-1] if len(req) else ""))
    print("   %d witness rows, %d of them constants; ready at some request (lag of one request) %d = %.1f %%, behind the last request %d = %.1f %%" % (
        nw, consts, int(ready[-1]), 100.0 * int(ready[-1]) / max(nw, 1), nw - int(ready[-1]), 100.0 * (nw - int(ready[-1])) / max(nw, 1)))
    print("   divider waves' share n_inline = %d rows = %.1f %% in %d passes of %d rows x %d sets; the pack kernel takes %d" % (
        n_inline, 100.0 * n_inline / max(nw, 1), (n_inline + blob.G - 1) // blob.G, blob.G, blob.T, nw - n_inline))
