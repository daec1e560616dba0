"""The thread decode of the all-level stage kernels (r1cs/ptau_internal.hpp's level_butterfly: setup_ptau.hip's
idft_levels_stage_kernel and contribute.hip's fr_levels_stage_kernel take their level, group and twiddle index from it) where
there is no GPU.  tests/native/level_layout_host.cc decodes every thread of every stage for the top levels 1 to 16, under ASan
and UBSan, and checks the partition, the two thread layouts and the bounds of the slots and of the twiddle index; this module
holds the program's counts against the closed forms: stage s of a launch with the top level `top` has 2^top - 2^s butterflies
(2^(m-1) in each level m in (s, top]) and 2^s idle threads, twiddle indices up to 2^s - 1, and one twiddle index per wave while
top - s >= 6."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
TOPS = range(1, 17)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """the program's (return code, stdout, stderr): a stand-alone CPU program, no device"""
    exe = str(tmp_path_factory.mktemp("level_layout_host") / "level_layout_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(ROCM, "include"), "-o", exe, os.path.join(ROOT, "tests", "native", "level_layout_host.cc")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    return out.returncode, out.stdout, out.stderr


def test_the_sanitized_run_is_clean_and_finds_no_violation(run):
    rc, out, err = run
    assert rc == 0 and not err, out[-2000:] + err[-4000:]
    assert not [line for line in out.splitlines() if line.startswith("FAIL")]
    assert out.splitlines()[-1] == "failures 0"


def test_every_stage_has_the_butterflies_of_its_levels(run):
    """one line per (top, s), in order: the layout, 2^top - 2^s butterflies, 2^s idle threads, every k below 2^s and the top level
    reached, and every wave of a wave-uniform stage compared"""
    lines = [line.split() for line in run[1].splitlines() if not line.startswith(("FAIL", "failures"))]
    want = []
    for top in TOPS:
        for s in range(top):
            by_k = top - s >= 6
            want.append([str(top), str(s), "wave" if by_k else "lane", str((1 << top) - (1 << s)), str(1 << s), str((1 << s) - 1), str(top),
                         str((1 << top) // 64 if by_k else 0)])
    assert lines == want
