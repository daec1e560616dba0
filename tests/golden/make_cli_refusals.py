"""Records what the eight command-line tools of circom-witnesscalc_amd/r1cs/ answer when they refuse their arguments or their
input files: (args, exit status, stdout, stderr) of every invocation of TABLE, into cli_refusals.json in this directory (run
from the repo root: python tests/golden/make_cli_refusals.py [--bin DIR], DIR holding the built tools).  Every invocation ends
before the device is touched, so the recording needs no GPU; it runs in a temporary working directory with relative file names,
and the directory of the binaries, which some usage texts echo from argv[0], is replaced by BIN_MARK: the recording does not
depend on where it was made.  tests/test_cli_refusals_host.py replays TABLE against the built tools and compares all three fields.
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import contribution_fixtures as CF  # noqa: E402
from tests import groth16_fixtures as GF  # noqa: E402
from tests import ptau_fixtures as PF  # noqa: E402
from tests import r1cs_fixtures as F  # noqa: E402
from tests import zkey_coefs_fixtures as ZF  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDING = os.path.join(HERE, "cli_refusals.json")
BIN_MARK = "<bin>"
CON = ([(1, 1)], [(2, 1)], [(3, 1)])  # w1 w2 = w3
BAD = ("missing.bin", "empty.bin", "three.bin")  # no such file, no byte, b"abc"


def secret_files(n):
    """{name: text} of the files of `n` secrets that the table tries"""
    good = ["3", "5", "7", "11", "13"][:n]
    line = lambda toks: " ".join(toks) + "\n"  # noqa: E731
    return {
        "empty": "",
        "blank": " \n\t\r\n",
        "few": line(good[:-1]),
        "many": line(good + ["17"]),
        "bad_first": line(["3x"] + good[1:]),
        "bad_last": line(good[:-1] + ["1e3"]),
        "plus": line(["+3"] + good[1:]),
        "two256": line(good[:-1] + [str(1 << 256)]),
        "max": line(good[:-1] + [str((1 << 256) - 1)]),         # the parser takes it; the library refuses it: not below r
        "crlf_tabs": "\t" + "\r\n\t".join(good[:-1] + ["0"]) + "\r\n",  # likewise, for its 0
    }


def write_files():
    """the inputs, into the working directory"""
    key = GF.Trapdoor([CON], 4, 0, seed=5).zkey
    blank = ZF.join([(i, CF.NO_RECORDS if i == 10 else b) for i, b in ZF.sections(key)])  # a key that takes contributions
    files = {"c.r1cs": F.write_r1cs(4, [CON]), "k.zkey": blank, "a.ptau": PF.write_ptau(2, 5, 7, 11), "w.wtns": ZF.wtns_image([1, 3, 5, 15]),
             "empty.bin": b"", "three.bin": b"abc", "obj.json": b"{}", "list.json": b"[]",
             "b32.bin": bytes(32), "b64.bin": bytes(64), "b96.bin": bytes(96), "b128.bin": bytes(128)}
    for n in (1, 3, 5):
        for name, text in secret_files(n).items():
            files["s%d_%s.txt" % (n, name)] = text.encode()
    for name, data in files.items():
        with open(name, "wb") as f:
            f.write(data)


def each_bad(tool, args, positions):
    """the invocation with each of BAD at each of `positions` of args in turn"""
    return [[tool] + args[:p] + [bad] + args[p + 1:] for p in positions for bad in BAD]


def table():
    t = []
    # -- arguments: none, a wrong number of paths, an unknown option, options that exclude each other
    for tool in ("check-witness", "witness-h", "groth16-prove", "groth16-verify", "groth16-setup", "groth16-contribute", "powersoftau", "kzg"):
        t += [[tool], [tool, "one"], [tool, "-x", "a", "b"], [tool, "a", "b", "c", "d", "e", "f", "g"]]
    t += [["groth16-prove", "--check-g2", "--check-g2", "k.zkey", "w.wtns", "p.json", "pub.json"],
          ["groth16-verify", "--compressed", "a", "b"],
          ["groth16-setup", "--ptau", "a.ptau", "--trapdoor", "s5_max.txt", "c.r1cs", "o.zkey"],
          ["groth16-setup", "--delta", "s1_max.txt", "c.r1cs", "o.zkey"],
          ["groth16-setup", "--lagrange", "file", "c.r1cs", "o.zkey"],
          ["groth16-setup", "--check-g2", "c.r1cs", "o.zkey"],
          ["groth16-setup", "--ptau", "a.ptau", "--check-g2", "--check-g2", "c.r1cs", "o.zkey"],
          ["groth16-setup", "--ptau", "a.ptau", "--lagrange", "maybe", "c.r1cs", "o.zkey"],
          ["groth16-setup", "--ptau"],
          ["groth16-setup", "--prepare-ptau", "a.ptau"],
          ["groth16-setup", "--check-lagrange", "a.ptau", "b.ptau"],
          ["groth16-setup", "--export-vk", "--compressed", "k.zkey"],
          ["groth16-contribute", "--verify", "--name", "n", "k.zkey"],
          ["groth16-contribute", "--verify", "--delta", "s1_max.txt", "k.zkey"],
          ["groth16-contribute", "--verify", "--verify-step", "k.zkey"],
          ["groth16-contribute", "--beacon", "--delta", "s1_max.txt", "k.zkey", "o.zkey", "00", "10"],
          ["groth16-contribute", "--require-beacon", "k.zkey", "o.zkey"],
          ["groth16-contribute", "--skip-records", "k.zkey", "o.zkey"],
          ["groth16-contribute", "--verify-key", "--lagrange", "maybe", "c.r1cs", "a.ptau", "k.zkey"],
          ["groth16-contribute", "--name", "n" * 256, "k.zkey", "o.zkey"],
          ["powersoftau", "renew", "2", "o.ptau"],
          ["powersoftau", "verify", "--require-beacon"],
          ["powersoftau", "contribute", "--require-beacon", "a.ptau", "o.ptau"],
          ["powersoftau", "beacon", "--secrets", "s3_max.txt", "a.ptau", "o.ptau", "00", "10"],
          ["powersoftau", "verify", "--name", "n", "a.ptau"],
          ["powersoftau", "contribute", "--name", "n" * 256, "a.ptau", "o.ptau"],
          ["powersoftau", "beacon", "--name", "n" * 256, "a.ptau", "o.ptau", "00", "10"],
          ["kzg", "fold", "a.ptau", "b32.bin", "o.bin"],
          ["kzg", "commit", "a.ptau", "b32.bin"],
          ["kzg", "open-fold", "a.ptau", "b32.bin", "b32.bin", "y.bin", "w.bin"]]
    # -- input files: missing, empty and three bytes long, at each input position
    t += each_bad("check-witness", ["c.r1cs", "w.wtns"], (0, 1))
    t += each_bad("witness-h", ["c.r1cs", "w.wtns", "h.bin"], (0, 1))
    t += each_bad("groth16-prove", ["k.zkey", "w.wtns", "p.json", "pub.json"], (0, 1))
    t += each_bad("groth16-prove", ["c.r1cs", "k.zkey", "w.wtns", "p.json", "pub.json"], (0, 1, 2))
    t += each_bad("groth16-prove", ["--compressed", "--check-g2", "k.zkey", "w.wtns", "p.bin", "pub.json"], (2, 3))
    t += each_bad("groth16-verify", ["obj.json", "list.json", "obj.json"], (0, 1, 2))
    t += [["groth16-verify", "obj.json", "list.json", "obj.json"], ["groth16-verify", "list.json", "list.json", "obj.json"]]
    t += each_bad("groth16-verify", ["--compressed", "b128.bin", "list.json", "b128.bin"], (1, 2, 3))
    t += [["groth16-verify", "--compressed", "b128.bin", "list.json", "b128.bin"]]
    t += each_bad("groth16-setup", ["c.r1cs", "o.zkey"], (0,))
    t += each_bad("groth16-setup", ["--ptau", "a.ptau", "c.r1cs", "o.zkey"], (1, 2))
    t += each_bad("groth16-setup", ["--prepare-ptau", "a.ptau", "o.ptau"], (1,))
    t += each_bad("groth16-setup", ["--check-lagrange", "a.ptau"], (1,))
    t += each_bad("groth16-setup", ["--check-lagrange", "--domain-power", "2", "a.ptau"], (3,))
    t += each_bad("groth16-setup", ["--export-vk", "k.zkey", "vk.json"], (1,))
    t += each_bad("groth16-setup", ["--export-vk", "--compressed", "k.zkey", "vk.bin"], (2,))
    t += each_bad("groth16-contribute", ["k.zkey", "o.zkey"], (0,))
    t += each_bad("groth16-contribute", ["--beacon", "k.zkey", "o.zkey", "00", "10"], (1,))
    t += each_bad("groth16-contribute", ["--verify", "k.zkey"], (1,))
    t += each_bad("groth16-contribute", ["--verify", "--require-beacon", "k.zkey"], (2,))
    t += each_bad("groth16-contribute", ["--verify-step", "k.zkey", "k.zkey"], (1, 2))
    t += each_bad("groth16-contribute", ["--verify-key", "c.r1cs", "a.ptau", "k.zkey"], (1, 2, 3))
    t += each_bad("powersoftau", ["contribute", "a.ptau", "o.ptau"], (1,))
    t += each_bad("powersoftau", ["beacon", "a.ptau", "o.ptau", "00", "10"], (1,))
    t += each_bad("powersoftau", ["verify", "a.ptau"], (1,))
    t += each_bad("powersoftau", ["verify", "--skip-records", "--require-beacon", "a.ptau"], (3,))
    t += each_bad("powersoftau", ["verify-step", "a.ptau", "a.ptau"], (1, 2))
    # -- files of secrets
    for n, tool, args in ((5, "groth16-setup", ["--trapdoor", "%s", "c.r1cs", "o.zkey"]),
                          (1, "groth16-setup", ["--ptau", "a.ptau", "--delta", "%s", "c.r1cs", "o.zkey"]),
                          (1, "groth16-contribute", ["--delta", "%s", "k.zkey", "o.zkey"]),
                          (3, "powersoftau", ["contribute", "--secrets", "%s", "a.ptau", "o.ptau"])):
        for name in ["missing"] + list(secret_files(n)):
            t.append([tool] + [a % ("s%d_%s.txt" % (n, name)) if "%s" in a else a for a in args])
    # -- hex and numbers
    for hexa in ("", "abc", "0x00", "0g", "ab" * 256):
        t += [["powersoftau", "beacon", "a.ptau", "o.ptau", hexa, "10"], ["groth16-contribute", "--beacon", "k.zkey", "o.zkey", hexa, "10"]]
    for number in ("", "1x", "4294967296"):
        t += [["powersoftau", "beacon", "a.ptau", "o.ptau", "00", number], ["groth16-contribute", "--beacon", "k.zkey", "o.zkey", "00", number],
              ["powersoftau", "new", number, "o.ptau"], ["groth16-setup", "--check-lagrange", "--domain-power", number, "a.ptau"]]
    t += [["groth16-setup", "--check-lagrange", "--domain-power", "29", "a.ptau"],
          ["powersoftau", "beacon", "a.ptau", "o.ptau", "aBcD", "9"], ["groth16-contribute", "--beacon", "k.zkey", "o.zkey", "ab" * 255, "64"]]
    # -- kzg: the `.ptau`, then each size that read_sized and read_poly refuse
    t += each_bad("kzg", ["commit", "a.ptau", "b32.bin", "c.bin"], (1, 2))
    t += each_bad("kzg", ["open", "a.ptau", "b64.bin", "b32.bin", "y.bin", "w.bin"], (1, 2, 3))
    t += each_bad("kzg", ["verify", "a.ptau", "b64.bin", "b32.bin", "b32.bin", "b64.bin"], (1, 2, 3, 4, 5))
    t += each_bad("kzg", ["verify-fold", "a.ptau", "b128.bin", "b32.bin", "b32.bin", "b64.bin", "b64.bin"], (1, 2, 3, 4, 5, 6))
    t += each_bad("kzg", ["open-fold", "a.ptau", "b32.bin", "b32.bin", "ys.bin", "w.bin", "b64.bin", "b64.bin"], (1, 2, 3, 6, 7))
    t += [["kzg", "verify", "a.ptau", "b32.bin", "b32.bin", "b32.bin", "b64.bin"], ["kzg", "verify", "a.ptau", "b64.bin", "b64.bin", "b32.bin", "b64.bin"],
          ["kzg", "verify", "a.ptau", "b64.bin", "b32.bin", "b96.bin", "b64.bin"], ["kzg", "verify", "a.ptau", "b64.bin", "b32.bin", "b32.bin", "b96.bin"],
          ["kzg", "verify-fold", "a.ptau", "b96.bin", "b32.bin", "b32.bin", "b64.bin", "b64.bin"],
          ["kzg", "verify-fold", "a.ptau", "b128.bin", "b32.bin", "b32.bin", "b32.bin", "b64.bin"],
          ["kzg", "verify-fold", "a.ptau", "b128.bin", "b32.bin", "b64.bin", "b64.bin", "b64.bin"],
          ["kzg", "open-fold", "a.ptau", "b32.bin", "b32.bin", "ys.bin", "w.bin", "b64.bin", "b96.bin"],
          ["kzg", "open-fold", "a.ptau", "b64.bin", "b32.bin", "ys.bin", "w.bin", "b64.bin"],
          ["kzg", "open", "a.ptau", "b64.bin", "b64.bin", "y.bin", "w.bin"]]
    return t


def run_table(bin_dir):
    """[{args, status, stdout, stderr}] of table() run with the tools of bin_dir, in a fresh working directory"""
    bin_dir = os.path.abspath(bin_dir)
    here = os.getcwd()
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            write_files()
            for args in table():
                p = subprocess.run([os.path.join(bin_dir, args[0])] + args[1:], capture_output=True, timeout=120)
                text = lambda b: b.decode("utf-8", "replace").replace(bin_dir, BIN_MARK)  # noqa: E731
                out.append({"args": args, "status": p.returncode, "stdout": text(p.stdout), "stderr": text(p.stderr)})
            written = set(os.listdir(".")) & {"o.zkey", "o.ptau", "o.bin", "h.bin", "p.json", "p.bin", "pub.json", "vk.json", "vk.bin", "c.bin", "y.bin",
                                              "ys.bin", "w.bin"}
            assert not written, "a refusal wrote an output file: %s" % sorted(written)
        finally:
            os.chdir(here)
    return out


if __name__ == "__main__":
    bin_dir = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--bin" else os.path.join(ROOT, "circom-witnesscalc_amd")
    records = run_table(bin_dir)
    with open(RECORDING, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")
    print("%d invocations recorded in %s" % (len(records), RECORDING))
