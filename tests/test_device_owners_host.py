"""The owners of device memory, streams and events (r1cs/device_owners.hpp) where there is no device: a stand-alone program
(tests/native/device_owners_host.cc, -fsanitize=address,undefined, linked against the HIP runtime) drives every owner through
its failure path, since without a device every allocation and every stream or event creation fails.  A failed call must leave
the owner empty and report the error; moves leave the source empty; reset and destruction of empty owners are clean.  Where a
device is visible the program has nothing to unwind and the test skips itself."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("device_owners_host") / "device_owners_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-self-move", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "device_owners_host.cc"), "-L" + os.path.join(ROCM, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROCM, "lib")])
    return exe


def test_owners_unwind_cleanly_without_a_device(host_program):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([host_program], capture_output=True, text=True, env=env, timeout=120)
    if out.stdout.strip() == "DEVICE":
        pytest.skip("a HIP device is visible: no allocation fails, so there is nothing to unwind")
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == 1 and lines[0].startswith("OK "), out.stdout
    assert int(lines[0].split()[1]) >= 47  # every section ran
