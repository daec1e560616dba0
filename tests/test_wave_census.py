"""The wave census (gwb_wave_census, tools/gpu_wave_census.py): the diagnostic that says which waves of an interpreter launch share a
SIMD.  CPU: the product library refuses it, the report counts what it is given.  GPU: the diagnostic library fills it for the
workgroup shapes of a two-stream divider program."""
import ctypes
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cwc_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = cwc_import.load().graphgen.circuits


def test_product_library_refuses_the_census(pkg):
    g = pkg.Graph(C.build_gadgets().to_bin())
    out = np.zeros(3 * 8192, dtype=np.uint64)
    st = pkg.GwStatus()
    L = pkg.lib()
    rc = L.gwb_wave_census(g._h, None, 1, None, None, out.ctypes.data, out.size, ctypes.byref(st))
    assert rc == 1 and "diagnostic library" in ctypes.string_at(st.error_msg).decode()
    L.gwb_free_status(ctypes.byref(st))
    rc = L.gwb_wave_census(g._h, None, 1, None, None, out.ctypes.data, 10, ctypes.byref(st))
    assert rc == 1 and "too small" in ctypes.string_at(st.error_msg).decode()
    L.gwb_free_status(ctypes.byref(st))
    assert not out.any()


def test_report_counts_waves_per_simd():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gpu_wave_census
    recs = []
    for wg in range(2):  # eight-wave workgroups [A.s0, A.s1, B.s0, B.s1, four dividers]: waves w and w + 4 on one SIMD
        for w in range(8):
            recs.append({"workgroup": wg, "wave": w, "xcc": 0, "se": 0, "sh": 0, "cu": wg, "simd": w % 4, "divider": int(w >= 4), "stream": w % 2,
                         "has_tile": 1, "start": 1000 + w, "end": 5000 + 100 * w})
    buf = io.StringIO()
    gpu_wave_census.report(recs, out=buf)
    text = buf.getvalue()
    assert "waves 16  workgroups 2  CUs used 2  SIMDs used 8; SIMDs holding n waves: 2: 8" in text
    assert "SIMDs holding {div0 + s0}: 4" in text and "SIMDs holding {div1 + s1}: 4" in text
    assert "waves alone on their SIMD: none" in text


@pytest.mark.gpu
@pytest.mark.parametrize("tiles_per_wg", ["1", "2"])
def test_census_of_a_two_stream_divider_program(pkg, tiles_per_wg):
    """Every wave of the launch reports once, under its role.  (Where the dispatcher puts them is printed, not asserted: it is the
    hardware's choice.)"""
    if not os.path.exists(pkg.DIAG_LIB_PATH):
        pkg.build(diag=True)
    env = dict(os.environ, PROBE_B="1024", CWC_LIB_PATH=pkg.DIAG_LIB_PATH, CWC_STREAM_TILES_PER_WORKGROUP=tiles_per_wg)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gpu_wave_census.py"), "0x902"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    m = re.search(r"waves (\d+)  workgroups (\d+)  CUs used (\d+)", r.stdout)
    assert m, r.stdout
    # 512 tiles x (two streams + two divider waves)
    assert int(m.group(1)) == 2048 and int(m.group(2)) == (512 if tiles_per_wg == "1" else 256), r.stdout
    for role in ("s0", "s1", "div0", "div1"):
        assert re.search(r"^   %s\s+waves\s+512 " % role, r.stdout, re.M), r.stdout
