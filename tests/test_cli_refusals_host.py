"""The refusals of the eight command-line tools of circom-witnesscalc_amd/r1cs/ against their recording (tests/golden/cli_refusals.json,
made by tests/golden/make_cli_refusals.py): the same table of invocations, run against the built tools, gives the same exit status,
stdout and stderr, byte for byte.  Every invocation ends before the device is touched.  And r1cs/cli_common.hpp, the tools' shared
helpers, alone under ASan and UBSan (tests/native/cli_common_main.cc)."""
import importlib.util
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "circom-witnesscalc_amd")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_cli_refusals", os.path.join(ROOT, "tests", "golden", "make_cli_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_tools_refuse_as_recorded():
    rec = _recorder()
    with open(rec.RECORDING) as f:
        want = json.load(f)
    got = rec.run_table(BIN)
    assert [w["args"] for w in want] == [g["args"] for g in got], "the table and the recording differ: record again"
    assert len(want) > 300 and all(w["status"] == 2 for w in want)
    differ = [(w, g) for w, g in zip(want, got) if w != g]
    assert not differ, "%d invocations differ, the first: recorded %r, got %r" % (len(differ), differ[0][0], differ[0][1])


def test_cli_common_hpp_under_sanitizers(tmp_path):
    """parse_secret_decimals, parse_decimal and decimal at 0, 2^256 - 1, 2^256 and 78 nines, at each count mismatch, with the output
    untouched on refusal; parse_hex, parse_u32, Mapped and write_file at their edges: the program checks them itself and prints ok"""
    exe = str(tmp_path / "cli_common_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "cli_common_main.cc")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and not out.stderr and out.stdout.endswith("ok\n"), out.stdout[-2000:] + out.stderr[-4000:]
