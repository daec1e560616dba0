"""Are two builds of the library the same compiler?  Prints the SHA-256 of the exported program blob of small generated circuits
at a few program keys, with no knob set and with one compiler knob at a time set (a new handle per knob).  Host only.  Run it
once per build and compare the outputs (profiles/knobs_blob_identity.txt holds the two lists of the knobs-snapshot change):

    CWC_LIB_PATH=<parent build>/libcircom_witnesscalc_amd.so python tools/knobs_blob_identity.py > parent.txt
    python tools/knobs_blob_identity.py > new.txt && diff parent.txt new.txt

A key a circuit cannot take (a stream program of a graph with one independent part) is printed as such instead of a hash."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("CWC_PROGRAM_CACHE", "0")
import cwc_import

DIVIDER, STREAMS2, STREAMS4 = 0x100, 0x800, 0x1000
KEYS = [1, 2, 4, 2 | DIVIDER, 1 | STREAMS4, 2 | DIVIDER | STREAMS2]
KNOBS = [None, ("CWC_FUSE", "1001"), ("CWC_CONV_ALWAYS", "1"), ("CWC_CONV_ANY_WIDTH", "1"), ("CWC_NO_BIT_SCANS", "1"), ("CWC_RANDOM_EVAL", "1"),
         ("CWC_NO_LOAD_OPTIMIZE", "1"), ("CWC_WITNESS_SLOTS", "1"), ("CWC_NO_COOP_MUL", "1")]


def main():
    pkg = cwc_import.load()
    C = pkg.graphgen.circuits
    circuits = [("gadgets", C.build_gadgets()), ("poseidon3", C.build_poseidon(3)), ("random_dag5", C.build_random_dag(5, n_ops=300)),
                ("random_dag7_parts3", C.build_random_dag(7, n_ops=300, parts=3)), ("chain_heavy3", C.build_chain_heavy(3)),
                ("bigint_k3", C.build_bigint_class(k=3, rounds=2)), ("bigint_k8", C.build_bigint_class(k=8, rounds=2)),
                ("bigint_k8_100bit", C.build_bigint_class(k=8, rounds=2, n_bits=100)), ("bigint_k2", C.build_bigint_class(k=2, rounds=3)),
                ("bigint_k3_32bit", C.build_bigint_class(k=3, rounds=2, n_bits=32)),
                ("limb_product1", C.build_limb_product_variants(1)), ("limb_divisions", C.build_limb_graph_with_divisions()),
                ("limb_chains", C.build_limb_chains()), ("rsa_64_4", C.build_rsa_long_div_class(n=64, k=4, muls=2)),
                ("rsa_121_3", C.build_rsa_long_div_class(n=121, k=3, muls=2, range_checks=False))]
    circuits += [("bit_recurrence%d" % s, C.build_bit_recurrence_variants(s)) for s in (0, 6, 16, 22, 1062344085)]
    for knob in KNOBS:
        if knob:
            os.environ[knob[0]] = knob[1]
        for name, b in circuits:
            g = pkg.Graph(b.to_bin())
            for key in KEYS:
                try:
                    digest = hashlib.sha256(g.export_blob(key)).hexdigest()
                except pkg.WitnessCalcError as e:
                    if "one independent part" not in str(e):
                        raise
                    digest = "skipped: one independent part"
                print("%-22s %-20s key %#06x  %s" % ("%s=%s" % knob if knob else "(no knob)", name, key, digest), flush=True)
        if knob:
            del os.environ[knob[0]]


if __name__ == "__main__":
    main()
