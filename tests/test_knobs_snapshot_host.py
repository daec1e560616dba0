"""The CWC_* environment knobs of libcircom_witnesscalc_amd.so (csrc/knobs.hpp): one reader, one list, and a compiler that sees
the environment through its caller's snapshot only.  Host tests, no GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "circom-witnesscalc_amd", "csrc")


def test_only_knobs_cc_reads_the_environment():
    readers = [f for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f)) and "getenv" in open(os.path.join(CSRC, f), errors="replace").read()]
    assert readers == ["knobs.cc"]


def test_the_documented_knobs_are_the_ones_read():
    """The names in INTEGRATION.md's table of the library's knobs == the names knobs.cc reads."""
    read = set(re.findall(r'"(CWC_[A-Z0-9_]+)"', open(os.path.join(CSRC, "knobs.cc")).read()))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = doc[doc.index("<!-- knobs table: begin -->"):doc.index("<!-- knobs table: end -->")]
    documented = re.findall(r"^\| `(CWC_[A-Z0-9_]+)` \|", table, re.M)
    assert len(documented) == len(set(documented))
    assert set(documented) == read and len(read) == 74


def test_compiler_follows_the_snapshot_not_the_environment(tmp_path):
    """tests/native/knobs_snapshot_host.cc under ASan + UBSan: a snapshot taken with CWC_NO_BIT_SCANS set still holds on a worker
    thread after the variable is gone, and a snapshot taken without it is not changed by setting the variable afterwards."""
    exe = str(tmp_path / "knobs_snapshot_host")
    units = ["graph.cc", "knobs.cc", "compile.cc", "rewrite.cc", "costmodel.cc", "program_blob.cc", "optimize.cc", "graphgen.cc"]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "knobs_snapshot_host.cc")] + [os.path.join(CSRC, u) for u in units])
    env = {k: v for k, v in os.environ.items() if not k.startswith("CWC_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and out.stdout.strip() == "OK" and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
