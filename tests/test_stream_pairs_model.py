"""Host side of the two-tile workgroups of two-stream divider programs (pipeline.cc waves_per_workgroup, estimate_cycles,
candidate_keys): the compiler is untouched -- every program blob is the parent commit's, byte for byte -- the cost model offers
the shape for 257-512 tiles only and picks what it picked wherever no candidate falls in that range, and such programs run
through the program emulator like any other.  tests/golden/parent_programs_and_picks.json was written by the parent commit's build."""
import hashlib
import json
import os

import pytest

from oracle import model
import cwc_import
import program_emulator as pe

C = cwc_import.load().graphgen.circuits
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parent_programs_and_picks.json")))
DIVIDER, STREAMS2 = 0x100, 0x800
GRAPHS = {"authv2_class_0.15": lambda: C.build_authv2_class(scale=0.15), "gadgets": C.build_gadgets, "sha256_64": lambda: C.build_sha256(64),
          "authv2_class": C.build_authv2_class, "sha256_512": lambda: C.build_sha256(512)}


@pytest.mark.parametrize("name", sorted(GOLD["blob_sha256"]))
def test_every_program_blob_is_the_parents(pkg, name):
    g = pkg.Graph(GRAPHS[name]().to_bin())
    for key, want in GOLD["blob_sha256"][name].items():
        assert hashlib.sha256(bytes(g.export_blob(int(key, 16)))).hexdigest() == want, (name, key)


def _offered(batch):
    """does a candidate tile width of this batch have 257-512 tiles? (candidate_keys: the rule's width t0, from t0 / 4 to 2 t0)"""
    t0 = 1 if batch <= 256 else 2 if batch <= 1024 else 4
    while t0 < 64 and (batch + t0 - 1) // t0 > 2048:
        t0 *= 2
    t = max(1, t0 // 4) if t0 >= 4 else 1
    while t <= 2 * t0 and t <= 32:
        if 257 <= (batch + t - 1) // t <= 512:
            return True
        t *= 2
    return False


@pytest.mark.parametrize("name", sorted(GOLD["picks"]))
def test_choices_outside_the_new_range_are_the_parents(pkg, name):
    g = pkg.Graph(GRAPHS[name]().to_bin())
    outside = 0
    for b, want in GOLD["picks"][name].items():
        batch, got = int(b), g.pick_tile_width(int(b))
        if not _offered(batch):
            outside += 1
            assert got == want, (name, batch, hex(got), hex(want))
        elif got != want:  # a new choice is the new shape: two streams, a divider wave each, 257-512 tiles
            t = got & 0xff
            assert got & ~0xff == DIVIDER | STREAMS2 and 257 <= (batch + t - 1) // t <= 512, (name, batch, hex(got), hex(want))
    assert outside >= 8
    if name == "sha256_512":  # no divisions: nothing new is offered at all
        assert all(g.pick_tile_width(int(b)) == want for b, want in GOLD["picks"][name].items())


def test_headline_batch_takes_two_streams_on_the_authv2_class_graph(pkg):
    g = pkg.Graph(C.build_authv2_class().to_bin())
    assert g.pick_tile_width(1024) == 2 | DIVIDER | STREAMS2
    assert g.pick_tile_width(2048) == GOLD["picks"]["authv2_class"]["2048"]


@pytest.mark.parametrize("T", [1, 2, 4])
def test_two_stream_divider_programs_through_the_emulator(pkg, T):
    """authV2-class (scaled), gadget and a division-free graph: the blob of key T | divider | two streams gives the oracle model's
    witnesses; the graph without divisions or without independent parts compiles to what it compiles to today (golden hashes above)."""
    import random
    rnd = random.Random(T)
    field = lambda n: [1] + [rnd.randrange(model.M) for _ in range(n - 1)]
    bits = lambda n: [1] + [rnd.randrange(2) for _ in range(n - 1)]
    for mk, rows_of, n_rows in ((lambda: C.build_authv2_class(scale=0.05), field, 1), (C.build_gadgets, field, 3), (lambda: C.build_sha256(64), bits, 1)):
        data = mk().to_bin()
        g = pkg.Graph(data)
        nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
        blob = pe.Blob(g.export_blob(T | DIVIDER | STREAMS2))
        for _ in range(n_rows):
            row = rows_of(g.n_inputs)
            got, st = pe.run(blob, row)
            try:
                want = model.evaluate(nodes, row, wit)
            except Exception:  # (a panicking set of the gadget graph: the status says so)
                assert st != 0
                continue
            assert st == 0 and got == want


def test_inline_pack_switches_keep_the_choice_among_programs_they_act_on(pkg, monkeypatch):
    """While CWC_INLINE_PACK / CWC_INLINE_PACK_ROWS is set (A/B runs of the divider waves' pack through the automatic choice) the new
    offer is withheld: the choice is the parent's, a one-stream divider program at the headline batch."""
    data = C.build_authv2_class().to_bin()
    for name, value in (("CWC_INLINE_PACK", "0"), ("CWC_INLINE_PACK", "1"), ("CWC_INLINE_PACK_ROWS", "60000")):
        monkeypatch.setenv(name, value)
        g = pkg.Graph(data)
        for b in ("768", "1024"):
            assert g.pick_tile_width(int(b)) == GOLD["picks"]["authv2_class"][b], (name, value, b)
        monkeypatch.delenv(name)
    assert pkg.Graph(data).pick_tile_width(1024) == 2 | DIVIDER | STREAMS2
