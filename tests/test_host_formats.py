"""CPU-side tests of the product's host logic through the C-ABI (no GPU compute calls): `.bin` reader and
writer, inputs JSON, `.wtns` framing, error behaviour of gw_calc_witness, exported symbols, and the graph
compiler checked by emulating the exported program blob."""
import ctypes
import hashlib
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import model
import cwc_import
C = cwc_import.load().graphgen.circuits
import program_emulator as pe

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(pkg):
    L = pkg.lib()
    declared = set()
    for h in ("graph_witness.h", "graph_witness_batch.h"):
        txt = open(os.path.join(ROOT, "include", h)).read()
        declared |= set(re.findall(r"\b(gwb?_[a-z_0-9]+)\s*\(", txt))
    declared -= {"gw_free_status"}  # header-inline, as in the reference header
    assert declared == set(pkg.EXPORTED_SYMBOLS)
    for s in declared:
        assert getattr(L, s) is not None


def test_gw_calc_witness_argument_errors(pkg):
    # reference src/lib.rs:51-64 messages; these return before any device work
    L = pkg.lib()
    out, n, st = ctypes.c_void_p(), ctypes.c_size_t(), pkg.GwStatus()
    data = open(os.path.join(GOLD, "circuit1.bin"), "rb").read()
    cases = [((None, data, len(data)), "inputs is null"), ((b"{}", None, 5), "graph_data is null"),
             ((b"{}", data, 0), "graph_data_len is 0")]
    for (a, b, c), msg in cases:
        rc = L.gw_calc_witness(a, b, c, ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
        assert rc == 1 and st.code == 1
        assert ctypes.string_at(st.error_msg).decode() == msg
        L.gwb_free_status(ctypes.byref(st))
    # bad JSON classes -> "Failed to calculate witness: ..." (reference lib.rs:88-92)
    for bad, frag in [(b'[1]', "inputs must be an object"), (b'{"a": -1}', "not a positive integer"),
                      (b'{"a": "12x"}', "InputFieldNumberParseError"), (b'{"a": [[1]]}', "inputs must be a string: a"),
                      (b'{"a": true}', "value for key a must be"), (b'{"a": ', "invalid JSON"),
                      (b'\xff\xfe', "Failed to parse inputs")]:
        rc = L.gw_calc_witness(bad, data, len(data), ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
        assert rc == 1
        assert frag in ctypes.string_at(st.error_msg).decode(), bad
        L.gwb_free_status(ctypes.byref(st))
    # malformed graphs (reference panics at lib.rs:130)
    for g in (b"not a graph at all......", data[:40], b"wtns.graph.001" + (2 ** 40).to_bytes(8, "little")):
        rc = L.gw_calc_witness(b'{"a":1}', g, len(g), ctypes.byref(out), ctypes.byref(n), ctypes.byref(st))
        assert rc == 1 and b"Failed to calculate witness" in ctypes.string_at(st.error_msg)
        L.gwb_free_status(ctypes.byref(st))


def test_bin_reader_and_writer_roundtrip(pkg):
    from tools.graphgen.pywriter import serialize_graph
    for b in (C.build_circuit1(), C.build_gadgets(), C.build_poseidon(2), C.build_random_dag(5, n_ops=200)):
        data = b.to_bin()                                   # the product's writer, through the C-ABI producer
        assert data == serialize_graph(*b.finalize())       # ... against the independent pure-Python writer
        g = pkg.Graph(data)
        nodes, wit, ins = model.deserialize_witnesscalc_graph(data)
        assert g.n_nodes == len(nodes) and g.n_witness == len(wit)
        assert g.n_inputs == model.get_inputs_size(nodes)
        assert g.n_op == sum(1 for n in nodes if n[0] in ("Uno", "Duo", "Tres"))
        # serialize_witnesscalc_graph reproduces the reference writer's bytes (storage.rs:137-183)
        assert g.serialize() == data
    # circuit1 fixture bytes
    assert pkg.Graph(open(os.path.join(GOLD, "circuit1.bin"), "rb").read()).serialize() == open(os.path.join(GOLD, "circuit1.bin"), "rb").read()


def test_c_abi_graph_producer(pkg):
    """gwb_builder_* is the producer side of the container (what build-circuit does with its Vec<Node>,
    reference src/storage.rs:137-183 / :50-91).  All five node variants of the reference's round-trip test
    (src/storage.rs:344-389) through the product writer: every record's bytes are the framing vectors of SURVEY 8(a) a13
    / the independent Python writer's, the trailing u64 points at the metadata record, the oracle's reader gets the same
    graph back; errors are sticky and reported by finish."""
    import ctypes
    import json
    import struct
    from tools.graphgen.pywriter import serialize_graph, encode_node, _varint
    G = pkg.graphgen.builder
    nodes = [("Input", 0), ("Const", 1), ("Uno", "Id", 1), ("Duo", "Mul", 0, 2), ("Tres", "TernCond", 1, 2, 3),
             ("Const", (1 << 200) + 5), ("Uno", "Neg", 5), ("Duo", "Bxor", 6, 3)]
    wit, ins = [4, 1, 7], {"sig1": (1, 3), "sig2": (5, 1)}
    data = G.write_bin(nodes, wit, ins)
    assert data == serialize_graph(nodes, wit, ins)
    got_nodes, got_wit, got_ins = model.deserialize_witnesscalc_graph(data)
    assert [tuple(n) for n in got_nodes] == nodes and list(got_wit) == wit and dict(got_ins) == ins
    pos = 14 + 8
    for n in nodes:  # record by record
        body = encode_node(n)
        rec = _varint(len(body)) + body
        assert data[pos:pos + len(rec)] == rec, n
        pos += len(rec)
    assert struct.unpack_from("<Q", data, len(data) - 8)[0] == pos  # storage.rs:448-464
    # the framing vectors of the reference-style records (tests/golden/kat_ops.json) through the product writer
    kat = json.load(open(os.path.join(GOLD, "kat_ops.json")))["node_framing"]
    named = {"Input(0)": ("Input", 0), "Input(1)": ("Input", 1), "Input(2)": ("Input", 2), "Const(2)": ("Const", 2),
             "Mul(2,3)": ("Duo", "Mul", 2, 3), "Add(4,0)": ("Duo", "Add", 4, 0)}
    order = ["Input(0)", "Input(1)", "Input(2)", "Const(2)", "Mul(2,3)", "Add(4,0)"]
    out = G.write_bin([named[k] for k in order], [0], {})
    pos = 14 + 8
    for k in order:
        rec = bytes.fromhex(kat[k])
        assert out[pos:pos + len(rec)] == rec, k
        pos += len(rec)
    # constants are field elements: a long / large byte string is reduced as the reader reduces it (storage.rs:28)
    big = (model.M * 3 + 9) << 8
    out = G.write_bin([("Const", big)], [0], {})
    assert model.deserialize_witnesscalc_graph(out)[0][0] == ("Const", big % model.M)
    # errors: forward reference, unknown operation code, witness beyond the graph -- sticky, reported by finish
    with pytest.raises(pkg.WitnessCalcError, match="references node 4 that is not before it"):
        G.write_bin([("Input", 0), ("Const", 1), ("Uno", "Id", 4)], [0], {})
    with pytest.raises(pkg.WitnessCalcError, match="witness signal references node 9"):
        G.write_bin([("Input", 0)], [9], {})
    L = pkg.lib()
    b = L.gwb_builder_new()
    try:
        assert L.gwb_builder_input(b, 0) == 0 and L.gwb_builder_duo(b, 20, 0, 0) == 0xFFFFFFFF  # (OP_BITX is not a wire code)
        assert L.gwb_builder_input(b, 1) == 0xFFFFFFFF and L.gwb_builder_node_count(b) == 1
        out_p, n, st = ctypes.c_void_p(), ctypes.c_size_t(), pkg.GwStatus()
        assert L.gwb_builder_finish(b, ctypes.byref(out_p), ctypes.byref(n), ctypes.byref(st)) == 1
        assert b"unknown DuoOp code 20" in ctypes.string_at(st.error_msg)
        L.gwb_free_status(ctypes.byref(st))
    finally:
        L.gwb_builder_free(b)


def test_bin_reader_accepts_unpacked_witness_and_long_constants(pkg):
    from tools.graphgen.pywriter import _varint, _field_bytes, _field_varint, encode_node
    import struct
    nodes = [("Const", 0), ("Input", 0), ("Input", 1), ("Duo", "Add", 2, 0)]
    out = bytearray(b"wtns.graph.001") + struct.pack("<Q", len(nodes))
    # constant longer than 32 bytes and >= r: reduced mod r on load (storage.rs:28)
    big = (model.M * 7 + 5) << 16
    body = _field_bytes(2, _field_bytes(1, _field_bytes(1, big.to_bytes(40, "little"))))
    out += _varint(len(body)) + body
    for n in nodes[1:]:
        body = encode_node(n)
        out += _varint(len(body)) + body
    md = b"".join(_varint((1 << 3) | 0) + _varint(w) for w in (1, 3, 0))  # unpacked repeated uint32
    md += _field_bytes(2, _field_bytes(1, b"a") + _field_bytes(2, _field_varint(1, 1) + _field_varint(2, 1)))
    md_off = len(out)
    out += _varint(len(md)) + md + struct.pack("<Q", md_off)
    g = pkg.Graph(bytes(out))
    assert (g.n_nodes, g.n_witness, g.n_inputs) == (4, 3, 2)
    n2, w2, i2 = model.deserialize_witnesscalc_graph(bytes(out))
    assert w2 == [1, 3, 0] and i2 == {"a": (1, 1)} and n2[0] == ("Const", big % model.M)
    blob = pe.Blob(g.export_blob(64))
    assert pe.run(blob, [1, 9])[0] == [1, (9 + big) % model.M, big % model.M]


def test_graph_validation_errors(pkg):
    from tools.graphgen.pywriter import serialize_graph
    bad = [
        ([("Input", 0), ("Duo", "Add", 0, 1)], [0], "not before it"),          # forward reference
        ([("Input", 0), ("Duo", "Pow", 0, 0)], [0], "Pow"),                     # graph.rs:141-142
        ([("Input", 0), ("Uno", "Id", 0)], [0], "Id"),                          # graph.rs:195
        ([("Input", 0)], [3], "witness signal"),
        # the graph of the reference's storage round-trip test (storage.rs:421-430) is not evaluable: rejected at load
        ([("Input", 0), ("Const", 1), ("Uno", "Id", 4), ("Duo", "Mul", 5, 6), ("Tres", "TernCond", 7, 8, 9)], [4, 1], "not before it"),
    ]
    for nodes, wit, frag in bad:
        with pytest.raises(pkg.WitnessCalcError, match=frag):
            pkg.Graph(serialize_graph(nodes, wit, {}))


def test_inputs_from_json_matches_reference_semantics(pkg):
    b = C.build_gadgets()
    g = pkg.Graph(b.to_bin())
    nodes, wit, ins = model.deserialize_witnesscalc_graph(b.to_bin())
    good = ['{"x": "123", "y": 7, "arr": ["1", 2, "3", 4]}', '{"x": 18446744073709551615, "arr": [1,2,3,4]}',
            '{"y": "%d"}' % (2 ** 256 - 1), '{"x":"1","x":"2"}', '{ "x" : "1_000" }', '{}',
            '{"\\u0078": "5"}', '{"y": ""}']
    for txt in good:
        row = g.inputs_from_json(txt)
        buf = model.get_inputs_buffer(g.n_inputs)
        model.populate_inputs(model.deserialize_inputs(txt), ins, buf)
        assert [int.from_bytes(row[i].tobytes(), "little") for i in range(g.n_inputs)] == buf, txt
    bad = ['{"x": 18446744073709551616}', '{"x": 1e3}', '{"x": "%d"}' % 2 ** 256, '{"nope": 1}', '{"arr": [1,2,3]}',
           '{"x": {"a":1}}', '{"x": [1, null]}', '{"x": 01}', '{"x": "1",}', "{'x': 1}", '{"x": "+1"}']
    for txt in bad:
        with pytest.raises(pkg.WitnessCalcError):
            g.inputs_from_json(txt)
    # reference lib.rs:259-271 vector: keys unknown to this graph -> reference panics, here an error; parse itself is
    # covered through the graph of matching shape
    import cwc_import
    Builder = cwc_import.load().graphgen.builder.Builder
    bb = Builder()
    k1 = bb.input("key1", 3); k2 = bb.input("key2"); k3 = bb.input("key3")
    for h in k1 + k2 + k3:
        bb.signal(h)
    g2 = pkg.Graph(bb.to_bin())
    kat = json.load(open(os.path.join(GOLD, "kat_ops.json")))["inputs_json"]
    row = g2.inputs_from_json(kat["text"])
    assert [int.from_bytes(row[i].tobytes(), "little") for i in range(6)] == [1, 123, 456, 100500, 789, 123123]


def test_wtns_framing(pkg):
    rnd = random.Random(2)
    for n in (0, 1, 4, 33):
        w = [rnd.randrange(model.M) for _ in range(n)]
        assert pkg.wtns_from_witness(w) == model.wtns_from_witness(w)
    assert pkg.wtns_from_witness([1, 31817, 105, 303]) == open(os.path.join(GOLD, "circuit1.wtns"), "rb").read()


DIVIDER = 0x100  # GWB_TILE_ASYNC_DIVIDER: programs for the asynchronous divider wave
GROUP = 0x200    # GWB_TILE_GROUP_DIVIDER: one divider wave per four interpreter waves
TRIPLE = 0x400   # GWB_TILE_TRIPLE_DIVIDER: one divider wave per three interpreter waves
STREAMS2 = 0x800   # GWB_TILE_STREAMS2: two wavefronts per tile, each over its share of the graph's independent parts
STREAMS4 = 0x1000  # GWB_TILE_STREAMS4: four


@pytest.mark.parametrize("tile", [1, 2, 4, 8, 16, 32, 64, 1 | DIVIDER, 2 | DIVIDER, 8 | DIVIDER, 32 | DIVIDER,
                                  1 | GROUP, 4 | GROUP, 32 | GROUP, 1 | TRIPLE, 2 | TRIPLE, 16 | TRIPLE,
                                  2 | STREAMS2, 1 | DIVIDER | STREAMS4, 4 | DIVIDER | STREAMS2, 8 | STREAMS4])
def test_graph_compiler_emulated(pkg, tile):
    """Level scheduling, bundling, slot reuse and operand encoding for every tile width and both division
    strategies (host logic only)."""
    rnd = random.Random(tile)
    key, tile = tile, tile & 0xff
    cases = [(C.build_gadgets(), 7), (C.build_poseidon(2), 3), (C.build_bigint_class(k=3, rounds=2), 8)] + \
            [(C.build_random_dag(s, n_ops=250, panic_free=(s % 2 == 0)), 7) for s in range(6)]
    for b, n_in in cases:
        data = b.to_bin()
        nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
        g = pkg.Graph(data)
        blob = pe.Blob(g.export_blob(key))
        assert blob.T == tile and blob.n_witness == len(wit) and blob.divider == (1 if key & DIVIDER else 4 if key & GROUP else 3 if key & TRIPLE else 0)
        assert blob.n_streams in ((1, 2) if key & STREAMS2 else (1, 4) if key & STREAMS4 else (1,))
        n_div = sum(1 for n in nodes if n[0] == "Duo" and n[1] == "Div")
        gone = blob.stats["n_folded"] + blob.stats["n_numbered"] + blob.stats["n_shaken"]  # (the load-time optimiser may remove divisions)
        if key & (DIVIDER | GROUP | TRIPLE):
            assert n_div - gone <= blob.stats["class_nodes"][9] == blob.stats["class_nodes"][10] <= n_div and blob.stats["class_nodes"][3] == 0
        else:
            assert n_div - gone <= blob.stats["class_nodes"][3] <= n_div and blob.n_div_requests == 0
        assert blob.stats["algorithmic_bytes_per_set"] == g.algorithmic_bytes_per_set
        arity = {"Uno": 1, "Duo": 2, "Tres": 3}
        want_bytes = 32 * (sum(arity[n[0]] + 1 for n in nodes if n[0] in arity) + 2 * sum(1 for n in nodes if n[0] == "Input") + 2 * len(wit))
        assert g.algorithmic_bytes_per_set == want_bytes
        for _ in range(2):
            row = [1] + [rnd.randrange(model.M) if rnd.random() < 0.6 else rnd.randrange(1 << 10) for _ in range(n_in - 1)]
            got, st = pe.run(blob, row)
            try:
                want = model.evaluate(nodes, row, wit)
            except model.ReferencePanic:
                assert st != 0
                continue
            assert st == 0 and got == want


def test_fused_narrow_chains_are_exact(pkg, monkeypatch):
    """Round 3: the compiler fuses (s * s) * m + c and a * b +- c chains near the critical path into single nodes of narrow
    bundles (class MULF; rewrite.cc fuse_narrow_chains).  With the fusion forced for every eligible chain (CWC_FUSE=1001)
    the emulator -- which computes on the stored words, Montgomery or canonical -- gives the reference's witnesses, for
    tile widths 1 and 2, with divider waves and as stream programs; the additions of canonical-form values read the
    canonical copies of their constants (the bug the first GPU soak of this class found)."""
    monkeypatch.setenv("CWC_FUSE", "1001")
    rnd = random.Random(11)
    total_fused = 0
    cases = [C.build_poseidon(2), C.build_chain_heavy(3), C.build_chain_heavy(9, n_chains=16), C.build_bigint_class(k=3, rounds=2)] + \
            [C.build_random_dag(s, n_ops=220, panic_free=True, parts=1 + s % 3) for s in range(8)]
    for b in cases:
        data = b.to_bin()
        nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
        g = pkg.Graph(data)
        for key in (1, 2, 1 | DIVIDER, 2 | STREAMS4):
            blob = pe.Blob(g.export_blob(key))
            total_fused += blob.stats["n_fused_nodes"]
            assert (blob.stats["class_bundles"][13] > 0) == (blob.stats["n_fused_nodes"] > 0)
            row = [1] + [rnd.randrange(model.M) if rnd.random() < 0.6 else rnd.randrange(1 << 10) for _ in range(blob.n_inputs - 1)]
            got, st = pe.run(blob, row)
            assert st == 0 and got == model.evaluate(nodes, row, wit)
    assert total_fused > 200
    # wider tiles have no fused bundles (the lane layout is that of the four-lane product, tile widths 1 and 2)
    assert pe.Blob(pkg.Graph(C.build_poseidon(2).to_bin()).export_blob(4)).stats["n_fused_nodes"] == 0


SCAN_CASES = [(64, 64, 10, 2, False, False), (1, 1, 5, 1, False, True), (33, 63, 40, 1, True, False), (128, 64, 7, 3, False, True), (129, 65, 6, 2, False, False),
              (253, 253, 4, 1, False, False), (32, 32, 70, 1, True, True), (100, 17, 9, 2, True, False), (64, 64, 33, 1, True, False)]
SCAN_POOL = [0, 1, 2, model.M - 1, (1 << 64) - 1, 1 << 64, (1 << 128) - 1, 1 << 128, 1 << 200, (1 << 32) - 1, 1 << 63]


def scan_rows(rnd, n_inputs, n_rows):
    """input rows for limb-chain graphs: uniform field elements (the general 256-bit paths), limb-sized values (the straight
    paths), edge values, and mixtures of the three"""
    rows = []
    for trial in range(n_rows):
        kind = trial % 4
        rows.append([1] + [rnd.randrange(model.M) if kind == 0 else rnd.randrange(1 << 64) if kind == 1 else rnd.choice(SCAN_POOL) if kind == 2
                           else rnd.choice([rnd.randrange(model.M), rnd.randrange(1 << 64), rnd.choice(SCAN_POOL)]) for _ in range(n_inputs - 1)])
    return rows


def test_convolution_columns_are_exact(pkg):
    """Round 4: the column sums of a k x k schoolbook limb product -- k^2 canonical products each read once by the Add tree of
    its column -- become 2k - 1 N_CONV nodes that ONE bundle computes (rewrite.cc detect_convolutions; class SCAN with
    HDR_SCAN_CONV).  The emulator runs the compiled programs of bigint-class graphs on the stored words: k = 2 .. 32 limbs, limb
    widths 32 / 64 / 100 / 130 bits, tile widths 1 and 2 (32 limbs fit tile width 1 only: 63 columns), inputs of every size;
    the programs hold no multiplication bundle any more, and a block whose products something else reads stays as it is."""
    rnd = random.Random(3)
    for k, rounds, nb, any_width in ((8, 3, 64, False), (4, 2, 64, False), (16, 2, 64, False), (32, 1, 64, False), (8, 2, 100, True), (5, 2, 130, True), (3, 2, 32, False), (2, 3, 64, False),
                                     (8, 2, 100, False)):
        b = C.build_bigint_class(k=k, rounds=rounds, n_bits=nb)
        data = b.to_bin()
        nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
        # (limbs that are not known to fit 64 bits keep their unfused products -- the bundle's rounds for such factors cost more --
        # unless CWC_CONV_ANY_WIDTH lifts the rule: the field-arithmetic rounds stay covered)
        os.environ.pop("CWC_CONV_ANY_WIDTH", None)
        if any_width:
            os.environ["CWC_CONV_ANY_WIDTH"] = "1"
        os.environ["CWC_CONV_ALWAYS"] = "1"   # (the unfused program competes and wins for the smallest products: below)
        g = pkg.Graph(data)
        for key in (1, 2):
            blob = pe.Blob(g.export_blob(key))
            fits = 2 * k - 1 <= 64 // key and (nb <= 64 or any_width)
            assert blob.stats["n_conv_products"] == (k * k * rounds if fits else 0), (k, key)
            assert (blob.stats["class_bundles"][1] == 0) == fits, "the limb products left the multiplication bundles"
            if nb == 64 and k >= 4:  # chain ends are steps too (the head without an incoming carry, the tail without an x, the division's head): 2k + 2k per round, no Idiv / Mod bundle left
                assert blob.stats["n_scan_steps"] == 4 * k * rounds and blob.stats["class_bundles"][7] == 0, (k, key, blob.stats["n_scan_steps"])
            for row in scan_rows(rnd, blob.n_inputs, 2 if k > 8 else 3):
                got, st = pe.run(blob, row)
                assert st == 0 and got == model.evaluate(nodes, row, wit), (k, key)
        assert pe.Blob(g.export_blob(4)).stats["n_conv_products"] == 0
        os.environ.pop("CWC_CONV_ANY_WIDTH", None)
        os.environ.pop("CWC_CONV_ALWAYS", None)
    # many small products side by side: the unfused program (a few full bundles for all of them) competes with one bundle per
    # product, and the cost model picks; CWC_CONV_ALWAYS=1 keeps the convolution bundles
    def blocks(n_blocks, k):
        b = cwc_import.load().graphgen.builder.Builder()
        xs, ys = b.input("x", n_blocks * k), b.input("y", n_blocks * k)
        m, base = b.const((1 << 64) - 1), b.const(1 << 64)
        xs, ys = [b.op("Band", v, m) for v in xs], [b.op("Band", v, m) for v in ys]
        for blk in range(n_blocks):
            cols = [None] * (2 * k - 1)
            for i in range(k):
                for j in range(k):
                    pr = b.mul(xs[blk * k + i], ys[blk * k + j])
                    cols[i + j] = pr if cols[i + j] is None else b.add(cols[i + j], pr)
            carry = b.const(0)
            for c in range(2 * k - 1):
                t = b.add(cols[c], carry)
                b.signal(b.op("Mod", t, base))
                carry = b.signal(b.op("Idiv", t, base))
        return b
    data = blocks(14, 3).to_bin()
    nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
    picked = pe.Blob(pkg.Graph(data).export_blob(1))
    os.environ["CWC_CONV_ALWAYS"] = "1"
    try:
        forced = pe.Blob(pkg.Graph(data).export_blob(1))
    finally:
        os.environ.pop("CWC_CONV_ALWAYS", None)
    assert forced.stats["n_conv_products"] == 14 * 9 and picked.stats["n_conv_products"] == 0 and picked.n_bundles < forced.n_bundles
    for blob in (picked, forced):
        for row in scan_rows(rnd, blob.n_inputs, 3):
            got, st = pe.run(blob, row)
            assert st == 0 and got == model.evaluate(nodes, row, wit)
    # the shapes the recognition has to tell apart (graphgen build_limb_product_variants: rectangular blocks, squares, shared factor
    # vectors, columns with an extra addend, products that are witness elements, a limb missing from a block, operand orders and
    # tree shapes): exact whatever becomes of them, with and without the competition of the unfused program
    n_conv = 0
    for seed in range(60):
        data = C.build_limb_product_variants(seed).to_bin()
        nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
        for always in (False, True):
            os.environ.pop("CWC_CONV_ALWAYS", None)
            if always:
                os.environ["CWC_CONV_ALWAYS"] = "1"
            try:
                g = pkg.Graph(data)
                for key in (1, 2) + ((2 | STREAMS4, 1 | STREAMS4) if seed % 3 == 0 else ()):  # (stream programs: a product's columns stay in one stream)
                    blob = pe.Blob(g.export_blob(key))
                    n_conv += blob.stats["n_conv_products"]
                    for row in scan_rows(rnd, blob.n_inputs, 2):
                        got, st = pe.run(blob, row)
                        assert st == 0 and got == model.evaluate(nodes, row, wit), (seed, key, always)
            finally:
                os.environ.pop("CWC_CONV_ALWAYS", None)
    assert n_conv > 300
    # A factor that depends on the block itself (round 4's advisor: x_1 = x_0 y_0 mod 2^64 -- the bundle would wait for x_1 and x_1 for
    # column 0): the block is left alone; and should a grouping that cannot be scheduled ever get through (here: with the dependency
    # check switched off), compile_program falls back to the program without convolution bundles instead of failing the graph.
    def dependent_block():
        b = cwc_import.load().graphgen.builder.Builder()
        xin, yin, cin = b.input("x", 3), b.input("y", 3), b.input("c", 40)
        m, base, zero = b.const((1 << 64) - 1), b.const(1 << 64), b.const(0)
        x0, x2 = b.op("Band", xin[0], m), b.op("Band", xin[2], m)
        y = [b.op("Band", v, m) for v in yin]
        p00 = b.mul(x0, y[0])
        x = [x0, b.op("Band", p00, m), x2]
        cols = [None] * 5
        for i in range(3):
            for j in range(3):
                pr = p00 if (i, j) == (0, 0) else b.mul(x[i], y[j])
                cols[i + j] = pr if cols[i + j] is None else b.add(cols[i + j], pr)
        for c in range(1, 5):
            b.signal(b.op("Band", cols[c], m))
        b.signal(x[1])
        carry = zero   # (an unrelated carry chain: the graph counts as a limb graph)
        for v in cin:
            t = b.add(b.op("Band", v, m), carry)
            b.signal(b.op("Mod", t, base))
            carry = b.signal(b.op("Idiv", t, base))
        return b
    data = dependent_block().to_bin()
    nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
    for skip_check in (False, True):
        os.environ.pop("CWC_CONV_SKIP_DEPENDENCY_CHECK", None)
        os.environ["CWC_CONV_ALWAYS"] = "1"
        if skip_check:
            os.environ["CWC_CONV_SKIP_DEPENDENCY_CHECK"] = "1"
        try:
            for key in (1, 2):
                blob = pe.Blob(pkg.Graph(data).export_blob(key))
                assert blob.stats["n_conv_products"] == 0 and blob.stats["n_scan_steps"] > 0
                for row in scan_rows(rnd, blob.n_inputs, 3):
                    got, st = pe.run(blob, row)
                    assert st == 0 and got == model.evaluate(nodes, row, wit)
        finally:
            os.environ.pop("CWC_CONV_SKIP_DEPENDENCY_CHECK", None)
            os.environ.pop("CWC_CONV_ALWAYS", None)
    # a limb graph that also holds field divisions: scan / convolution bundles beside in-line divisions or beside the requests to
    # a divider wave
    data = C.build_limb_graph_with_divisions().to_bin()
    nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
    g = pkg.Graph(data)
    for key in (1, 2, 1 | DIVIDER, 2 | DIVIDER, 1 | STREAMS4, 4):
        blob = pe.Blob(g.export_blob(key))
        limb_paths = key != 4
        assert (blob.stats["n_scan_steps"] > 0) == limb_paths and (blob.stats["n_conv_products"] > 0) == limb_paths, hex(key)
        assert (blob.stats["class_bundles"][9] > 0) == bool(key & DIVIDER), "division requests in the programs for divider waves only"
        for row in scan_rows(rnd, blob.n_inputs, 3):
            got, st = pe.run(blob, row)
            assert st == 0 and got == model.evaluate(nodes, row, wit), hex(key)
    # a product that a witness element names is no inner node: the block keeps its unfused nodes
    b = cwc_import.load().graphgen.builder.Builder()
    xs, ys = b.input("x", 3), b.input("y", 3)
    m = b.const((1 << 64) - 1)
    xs, ys = [b.op("Band", v, m) for v in xs], [b.op("Band", v, m) for v in ys]
    cols = [None] * 5
    for i in range(3):
        for j in range(3):
            pr = b.mul(xs[i], ys[j])
            if i == 1 and j == 1:
                b.signal(pr)
            cols[i + j] = pr if cols[i + j] is None else b.add(cols[i + j], pr)
    carry = b.const(0)
    base = b.const(1 << 64)
    for c in range(5):
        t = b.add(cols[c], carry)
        b.signal(b.op("Mod", t, base))
        carry = b.signal(b.op("Idiv", t, base))
    data = b.to_bin()
    nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
    blob = pe.Blob(pkg.Graph(data).export_blob(1))
    assert blob.stats["n_conv_products"] == 0
    for row in scan_rows(rnd, blob.n_inputs, 3):
        got, st = pe.run(blob, row)
        assert st == 0 and got == model.evaluate(nodes, row, wit)


def test_parallel_scan_algorithms_on_plain_integers():
    """The parallel forms of the scan recurrences (csrc/scan_gfx950.hpp scan_carry_parallel / scan_div_parallel) restated on
    plain integers, pair by pair, against the serial recurrences: the three-word column sums, the two local carry rounds, the
    lookahead as ONE integer addition over gate and generate / propagate bits (two bits per pair), the carry leaving a
    position; the segmented prefix of the maps r -> (r m + v) mod d and the quotient digits.  Random segment starts, all-ones
    runs, x up to 192 bits, divisors 1, 2, 2^63, 2^64 - 1."""
    B = 1 << 64

    def serial_carry(xs, starts, a0s):
        limb, carry, c = [], [], 0
        for p, x in enumerate(xs):
            t = x + (a0s[p] if starts[p] else c)
            limb.append(t % B)
            c = t // B
            carry.append(c)
        return limb, carry

    def par_carry(xs, starts, a0s):
        L = len(xs)
        xp = [xs[p] + (a0s[p] if starts[p] else 0) for p in range(L)]
        x0, x1, x2 = [v % B for v in xp], [(v >> 64) % B for v in xp], [v >> 128 for v in xp]
        prev = lambda a: [0 if starts[p] else v for p, v in enumerate([0] + a[:-1])]   # the previous pair's value, nothing at a segment's start
        y1, y2a = prev(x1), prev(x2)
        y2 = prev(y2a)
        s = [x0[p] + y1[p] + y2[p] for p in range(L)]
        lo, ov = [v % B for v in s], [v // B for v in s]
        u = [a + c for a, c in zip(lo, prev(ov))]
        lo2, w = [v % B for v in u], [v // B for v in u]
        z = [a + c for a, c in zip(lo2, prev(w))]
        gen, zz = [v >= B for v in z], [v % B for v in z]
        prop = [v == B - 1 for v in zz]
        a = b = 0
        for p in range(L):
            a |= (0 if starts[p] else 1) << (2 * p) | (1 if gen[p] or prop[p] else 0) << (2 * p + 1)
            b |= (1 if gen[p] else 0) << (2 * p + 1)
        cbits = (a + b) ^ a ^ b
        cin = [(cbits >> (2 * p + 1)) & 1 for p in range(L)]
        limb = [(zz[p] + cin[p]) % B for p in range(L)]
        cout = [1 if gen[p] or (prop[p] and cin[p]) else 0 for p in range(L)]
        return limb, [x1[p] + x2[p] * B + y2a[p] + ov[p] + w[p] + cout[p] for p in range(L)]

    def serial_div(xs, starts, a0s, ds):
        q, r, rem = [], [], 0
        for p, x in enumerate(xs):
            t = (a0s[p] if starts[p] else rem) * B + x
            q.append(t // ds[p])
            rem = t % ds[p]
            r.append(rem)
        return q, r

    def par_div(xs, starts, a0s, ds):
        L = len(xs)
        m = [0 if starts[p] else B % ds[p] for p in range(L)]
        v = [((a0s[p] if starts[p] else 0) * B + xs[p]) % ds[p] for p in range(L)]
        f = list(starts)
        delta = 1
        while delta < L:
            m2, v2, f2 = m[:], v[:], f[:]
            for p in range(delta, L):
                if not f[p]:
                    v2[p] = (v[p - delta] * m[p] + v[p]) % ds[p]
                    m2[p] = (m[p - delta] * m[p]) % ds[p]
                    f2[p] = f[p - delta]
            m, v, f = m2, v2, f2
            delta *= 2
        rin = [a0s[p] if starts[p] else v[p - 1] for p in range(L)]
        return [(rin[p] * B + xs[p]) // ds[p] for p in range(L)], v

    rnd = random.Random(4)

    def pick(bits):
        k = rnd.random()
        return (1 << bits) - 1 if k < 0.2 else 0 if k < 0.3 else ((1 << bits) - 1) ^ rnd.getrandbits(3) if k < 0.4 else rnd.getrandbits(bits)

    for trial in range(1500):
        L = rnd.choice([16, 32])
        starts = [p == 0 or rnd.random() < 0.1 for p in range(L)]
        bits = rnd.choice([64, 128, 133, 190])
        xs = [B - 1] * L if rnd.random() < 0.3 else [pick(rnd.choice([64, bits])) for _ in range(L)]
        a0s = [pick(rnd.choice([1, 64, 70, 190])) if starts[p] else None for p in range(L)]
        if all(xs[p] + (a0s[p] or 0) < (1 << 192) for p in range(L)):
            assert serial_carry(xs, starts, a0s) == par_carry(xs, starts, a0s)
        ds, d = [], 1
        for p in range(L):
            if starts[p]:
                d = rnd.choice([1, 2, 3, B - 1, B - 2, 1 << 63, (1 << 63) + 1, rnd.getrandbits(64) | 1, rnd.getrandbits(20) + 1])
            ds.append(d)
        xd = [pick(64) for _ in range(L)]
        a0d = [rnd.randrange(ds[p]) if starts[p] else None for p in range(L)]
        assert serial_div(xd, starts, a0d, ds) == par_div(xd, starts, a0d, ds)


def test_wide_register_scan_algorithms_on_plain_integers():
    """Round 5 (csrc/scan_gfx950.hpp scan_carry_parallel_wide, scan_bit_lookahead and the BORROW / LEX paths of kernels.hip) restated
    on plain integers against the serial recurrences: the carry chain's parallel form for registers of any width n <= 126
    (three digits below 2^n, x below min(2^(3n), 2^252)), and the two one-bit recurrences -- the borrow chain of a register-wise
    subtraction and the most-significant-difference comparison -- as generate / propagate bits resolved by one integer addition."""
    from oracle import model
    M = model.M

    def lookahead(starts, gen, prop):
        a = b = 0
        for p in range(len(starts)):
            a |= (0 if starts[p] else 1) << (2 * p) | (1 if gen[p] or prop[p] else 0) << (2 * p + 1)
            b |= (1 if gen[p] else 0) << (2 * p + 1)
        cbits = (a + b) ^ a ^ b
        return [(cbits >> (2 * p + 1)) & 1 for p in range(len(starts))]

    def serial_carry(n, xs, starts, a0s):
        limb, carry, c = [], [], 0
        for p, x in enumerate(xs):
            t = (x + (a0s[p] if starts[p] else c)) % M   # graph.rs:110, the field addition of the unfused step
            limb.append(t & ((1 << n) - 1))
            c = t >> n
            carry.append(c)
        return limb, carry

    def par_carry(n, xs, starts, a0s):
        B, L = 1 << n, len(xs)
        xp = [xs[p] + (a0s[p] if starts[p] else 0) for p in range(L)]
        d0, d1, d2 = [v % B for v in xp], [(v >> n) % B for v in xp], [v >> (2 * n) for v in xp]
        assert all(v < B for v in d2)
        prev = lambda a: [0 if starts[p] else v for p, v in enumerate([0] + a[:-1])]
        y1, y2a = prev(d1), prev(d2)
        y2 = prev(y2a)
        s = [d0[p] + y1[p] + y2[p] for p in range(L)]
        assert all(v < (1 << 128) for v in s)
        lo, ov = [v % B for v in s], [v >> n for v in s]
        u = [a + c for a, c in zip(lo, prev(ov))]
        lo2, w = [v % B for v in u], [(v >> n) & 1 for v in u]
        z = [a + c for a, c in zip(lo2, prev(w))]
        gen, prop = [(v >> n) & 1 == 1 for v in z], [v == B - 1 for v in z]
        cin = lookahead(starts, gen, prop)
        limb = [(z[p] + cin[p]) % B for p in range(L)]
        cout = [1 if gen[p] or (prop[p] and cin[p]) else 0 for p in range(L)]
        return limb, [d1[p] + y2a[p] + ov[p] + w[p] + cout[p] + (d2[p] << n) for p in range(L)]

    def serial_borrow(n, xs, ys, starts, a0s):
        out, acc, b = [], [], 0
        for p in range(len(xs)):
            bi = a0s[p] if starts[p] else b
            c = model.eval_duo("Geq", xs[p], (ys[p] + bi) % M)
            out.append((xs[p] - ys[p] - bi) % M if c else (xs[p] - ys[p] - bi + (1 << n)) % M)
            b = 0 if c else 1
            acc.append(b)
        return out, acc

    def par_borrow(n, xs, ys, starts, a0s):   # registers below 2^n
        L = len(xs)
        gen, prop = [xs[p] < ys[p] for p in range(L)], [xs[p] == ys[p] for p in range(L)]
        gs = [gen[p] or (starts[p] and prop[p] and a0s[p] == 1) for p in range(L)]
        cin = lookahead(starts, gs, prop)
        bi = [a0s[p] if starts[p] else cin[p] for p in range(L)]
        bout = [1 if gen[p] or (prop[p] and bi[p]) else 0 for p in range(L)]
        return [((xs[p] - ys[p] - bi[p]) + (bout[p] << n)) % (1 << 128) for p in range(L)], bout

    def serial_lex(kg, kl, xs, ys, starts, a0s):
        acc, b = [], 0
        for p in range(len(xs)):
            bi = a0s[p] if starts[p] else b
            b = kg if model.eval_duo("Gt", xs[p], ys[p]) else kl if model.eval_duo("Lt", xs[p], ys[p]) else bi
            acc.append(b)
        return acc

    def par_lex(kg, kl, xs, ys, starts, a0s):
        L = len(xs)
        gt, lt = [model.eval_duo("Gt", xs[p], ys[p]) for p in range(L)], [model.eval_duo("Lt", xs[p], ys[p]) for p in range(L)]
        gen = [bool((gt[p] and kg) or (lt[p] and kl)) for p in range(L)]
        prop = [not gt[p] and not lt[p] for p in range(L)]
        cin = lookahead(starts, [gen[p] or (starts[p] and prop[p] and a0s[p] == 1) for p in range(L)], prop)
        bi = [a0s[p] if starts[p] else cin[p] for p in range(L)]
        return [1 if gen[p] or (prop[p] and bi[p]) else 0 for p in range(L)]

    rnd = random.Random(12)

    def pick(bits):
        k = rnd.random()
        return (1 << bits) - 1 if k < 0.2 else 0 if k < 0.3 else ((1 << bits) - 1) ^ rnd.getrandbits(3) if k < 0.4 else rnd.getrandbits(bits)

    for trial in range(3000):
        L = rnd.choice([16, 32])
        n = rnd.choice([2, 7, 31, 32, 33, 55, 63, 65, 96, 100, 121, 126])
        starts = [p == 0 or rnd.random() < 0.1 for p in range(L)]
        top = min(3 * n, 252)
        xs = [(1 << n) - 1] * L if rnd.random() < 0.3 else [pick(rnd.choice([n, min(2 * n, top), top])) for _ in range(L)]
        a0s = [pick(rnd.choice([1, n, min(n + 6, top)])) if starts[p] else None for p in range(L)]
        if all(xs[p] + (a0s[p] or 0) < (1 << top) for p in range(L)):
            assert serial_carry(n, xs, starts, a0s) == par_carry(n, xs, starts, a0s), (n, trial)
        # one-bit recurrences on registers below 2^n, equal registers and borrows that ripple among them
        xr = [pick(n) & ((1 << n) - 1) for _ in range(L)]
        yr = [xr[p] if rnd.random() < 0.4 else pick(n) & ((1 << n) - 1) for p in range(L)]
        b0 = [rnd.randrange(2) if starts[p] else None for p in range(L)]
        assert serial_borrow(n, xr, yr, starts, b0) == par_borrow(n, xr, yr, starts, b0), (n, trial)
        kg, kl = rnd.randrange(2), rnd.randrange(2)
        # (the comparison is the reference's signed one: operands anywhere in the field)
        xf = [rnd.choice([xr[p], M - 1 - xr[p], rnd.randrange(M), M // 2, M // 2 + 1]) for p in range(L)]
        yf = [xf[p] if rnd.random() < 0.4 else rnd.choice([yr[p], M - 1 - yr[p], rnd.randrange(M), M // 2, M // 2 + 1]) for p in range(L)]
        assert serial_lex(kg, kl, xf, yf, starts, b0) == par_lex(kg, kl, xf, yf, starts, b0), (n, trial)


def test_native_generators_write_the_python_generators_bytes(pkg):
    """gwb_graphgen_bigint_class / gwb_graphgen_rsa_long_div_class (csrc/graphgen.cc: what the bench uses for BASELINE config 5's two
    ten-million-node graphs) emit the same nodes in the same order through the same layout rules as the Python generator library,
    their specification: the `.bin` bytes are equal over register widths, register counts, chain lengths, with and without range
    checks; the histogram of a loaded handle equals the Python builder's statistics."""
    for n, k, muls, rc in [(121, 17, 2, True), (64, 4, 18, True), (55, 5, 3, False), (12, 3, 2, True), (11, 2, 2, True), (126, 1, 2, True)]:
        assert C.build_rsa_long_div_class(n=n, k=k, muls=muls, range_checks=rc).to_bin() == pkg.graphgen_native("rsa", n=n, k=k, muls=muls, range_checks=rc), (n, k, muls, rc)
    for k, nb, rounds in [(8, 64, 4), (32, 64, 2), (3, 100, 2), (1, 16, 2)]:
        assert C.build_bigint_class(k=k, n_bits=nb, rounds=rounds).to_bin() == pkg.graphgen_native("bigint", k=k, n_bits=nb, rounds=rounds), (k, nb, rounds)
    b = C.build_rsa_long_div_class(n=64, k=4, muls=2)
    nodes, wit, _ = b.finalize()
    st = pkg.graphgen.builder.graph_stats(nodes, wit)
    g = pkg.Graph(pkg.graphgen_native("rsa", n=64, k=4, muls=2))
    assert g.op_histogram() == st["hist"] and g.n_nodes == st["N"] and g.depth == st["depth"]
    with pytest.raises(pkg.WitnessCalcError):
        pkg.graphgen_native("rsa", n=200, k=4, muls=1)


def test_rsa_long_div_class_generator_against_plain_integers(pkg):
    """graphgen.circuits.build_rsa_long_div_class restates circom-bigint's witness hints (schoolbook product with carries, long_div
    by a k-register divisor: short_div estimate, long_scalar_mult, long_gt, long_sub) node by node.  Outside anchor: for every
    chained multiplication the graph's q and r registers, evaluated by the C oracle, are divmod(a * b, p) on Python integers, and the
    range-check bits are the registers' bits -- over register widths 16 .. 126 and 1 .. 17 registers."""
    from oracle import cbind
    rnd = random.Random(31)
    for n, k, muls in [(121, 17, 2), (64, 4, 3), (55, 5, 18), (100, 3, 2), (126, 2, 2), (16, 3, 3), (121, 1, 2)]:
        data = C.build_rsa_long_div_class(n=n, k=k, muls=muls).to_bin()
        og = cbind.Graph(data)
        rows = [[1] + [rnd.randrange(model.M) if s % 2 == 0 else rnd.choice([0, 1, (1 << n) - 1, rnd.randrange(1 << n)]) for _ in range(2 * k)] for s in range(5)]
        want, st = og.evaluate_batch(cbind.ints_to_array(rows))
        assert not st.any()
        mask = (1 << n) - 1
        for s, row in enumerate(rows):
            w = [int.from_bytes(bytes(want[s][i]), "little") for i in range(want.shape[1])]
            xs, ps = [v & mask for v in row[1:1 + k]], [v & mask for v in row[1 + k:1 + 2 * k]]
            tb = max(n - 10, 1)
            ps[-1] = (row[2 * k] & ((1 << tb) - 1)) + (1 << tb)
            X, P = sum(v << (n * i) for i, v in enumerate(xs)), sum(v << (n * i) for i, v in enumerate(ps))
            assert w[0] == 1 and w[1:1 + k] == xs and w[1 + k:1 + 2 * k] == ps
            pos, acc = 1 + 2 * k, X
            for m in range(muls):
                Q, Rm = divmod(acc * (X if m % 17 == 16 else acc), P)
                regs = []
                for _i in range(2 * k):
                    regs.append(w[pos])
                    assert w[pos + 1:pos + 1 + n] == [(w[pos] >> j) & 1 for j in range(n)]
                    pos += n + 1
                assert sum(v << (n * i) for i, v in enumerate(regs[k:])) == Rm and sum(v << (n * i) for i, v in enumerate(regs[:k])) == Q % (1 << (n * k))
                acc = Rm
            assert pos == len(w)


def test_bit_recurrence_scans_are_exact(pkg, monkeypatch):
    """Round 5: the one-bit recurrences of multi-register integers -- the borrow chain of a register-wise subtraction, the
    comparison decided by the most significant differing register -- become scan bundles (rewrite.cc detect_bit_scans; steps
    recognised by VALUE through linear forms of the arms).  The emulator runs the exported programs of the RSA / long_div-class graph
    and of the variants generator (every comparison style, arm association, constant registers, kept / dropped last borrow, result
    bits, incoming booleans, registers of 2 .. 252 bits) against the Python model at tile widths 1, 2 (scan bundles) and 4, and with
    the recognition off; the RSA program must hold all three kinds of wide-register chains."""
    rnd = random.Random(41)

    kinds = pe.scan_kinds

    for n, k, muls in [(121, 17, 1), (64, 4, 2), (33, 6, 1), (121, 3, 2), (100, 6, 2)]:
        b = C.build_rsa_long_div_class(n=n, k=k, muls=muls, range_checks=(k < 17))
        nodes, wit, _ = b.finalize()
        g = pkg.Graph(b.to_bin())
        rows = [[1] + [rnd.randrange(model.M) if s == 0 else rnd.choice([0, 1, (1 << n) - 1, rnd.randrange(1 << n)]) for _ in range(2 * k)] for s in range(2)]
        for tw in (1, 2, 4, 1 | STREAMS4, 2 | DIVIDER | STREAMS4):
            try:
                blob = pe.Blob(g.export_blob(tw))
            except Exception as e:  # (the graph is one independent part: no stream program -- a plain selection whose ACC node sat in the prologue
                if "one independent part" in str(e):  # while its condition did not once made a bogus partition of it, found by the soak)
                    continue
                raise
            nb, nl, nc = kinds(blob)
            assert (nb > 0 and nl > 0 and nc > 0) == ((tw & 0xff) <= 2), (tw, nb, nl, nc)
            for row in rows:
                got, st = pe.run(blob, row)
                assert st == 0 and got == model.evaluate(nodes, row, wit)
    tot_b = tot_l = 0
    for seed in list(range(40)) + [1062344085, 346676167]:  # (the last two: round 5's soak found a selection step split between the prologue and a stream)
        b = C.build_bit_recurrence_variants(seed)
        nodes, wit, _ = b.finalize()
        data = b.to_bin()
        rows = [[1] + [rnd.choice([0, 1, rnd.getrandbits(rnd.choice([8, 64, 121, 128, 200])), rnd.randrange(model.M), model.M - 1 - rnd.getrandbits(20)]) for _ in range(b.n_inputs - 1)] for _s in range(2)]
        want = [model.evaluate(nodes, row, wit) for row in rows]
        for no_scans in (False, True) if seed % 8 == 0 else (False,):
            if no_scans:
                monkeypatch.setenv("CWC_NO_BIT_SCANS", "1")
            g = pkg.Graph(data)
            # (programs of four streams: a selection step's two nodes -- different operands, one bundle -- must not be torn apart by the prologue)
            for tw in (1, 2, 4) + ((1 | STREAMS4, 2 | DIVIDER | STREAMS4) if seed % 2 == 0 else ()):
                try:
                    blob = pe.Blob(g.export_blob(tw))
                except Exception as e:
                    if "one independent part" in str(e):
                        continue
                    raise
                nb, nl, _ = kinds(blob)
                assert not no_scans or (nb == 0 and nl == 0)
                if tw == 1:
                    tot_b, tot_l = tot_b + nb, tot_l + nl
                for row, w in zip(rows, want):
                    got, st = pe.run(blob, row)
                    assert st == 0 and got == w, (seed, tw)
            monkeypatch.delenv("CWC_NO_BIT_SCANS", raising=False)
    assert tot_b > 10 and tot_l > 10


def test_scan_chains_are_exact(pkg):
    """Round 4: the steps of serial limb recurrences -- carry chains `t = x + c; limb = t % 2^n; c' = t \\ 2^n`, remainder
    chains `t = r * 2^k + x; q = t \\ d; r' = t % d` -- become pairs of N_SCAN nodes that the scheduler places in consecutive
    pairs of node slots of scan bundles (class SCAN; rewrite.cc detect_scans).  The emulator runs the compiled programs on
    the stored words: every shift / base width, chains longer than a bundle, chains that fork, a step whose x is another
    step's output, operands outside the limb range, d == 0; tile widths 1 and 2, with divider waves and as stream programs
    (wider tiles keep the unfused nodes)."""
    rnd = random.Random(12)
    total = 0
    for case in SCAN_CASES:
        b = C.build_limb_chains(*case)
        data = b.to_bin()
        nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
        g = pkg.Graph(data)
        for key in (1, 2, 1 | DIVIDER, 2 | STREAMS4):
            blob = pe.Blob(g.export_blob(key))
            total += blob.stats["n_scan_steps"]
            assert (blob.stats["class_bundles"][14] > 0) == (blob.stats["n_scan_steps"] > 0) and blob.stats["class_bundles"][13] == 0
            assert blob.stats["n_scan_steps"] > 0, "scan bundles in programs with no or one divider wave per interpreter (kernels.hip launch_interp: which instances exist)"
            for row in scan_rows(rnd, blob.n_inputs, 4):
                got, st = pe.run(blob, row)
                assert st == 0 and got == model.evaluate(nodes, row, wit), (case, key)
        assert pe.Blob(g.export_blob(4)).stats["n_scan_steps"] == 0
    assert total > 1500
    # the bigint-class graph of BASELINE config 5: carry chains and the long division as scan bundles, a tenth of the bundles
    b = C.build_bigint_class(k=8, rounds=3)
    data = b.to_bin()
    nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
    g = pkg.Graph(data)
    for key in (1, 2):
        blob = pe.Blob(g.export_blob(key))
        assert blob.stats["n_scan_steps"] >= 80 and blob.n_bundles < 160
        for row in scan_rows(rnd, blob.n_inputs, 4):
            got, st = pe.run(blob, row)
            assert st == 0 and got == model.evaluate(nodes, row, wit)


def test_value_numbering_lists_and_overflow(pkg):
    """The tree-height reduction numbers its Add / Mul nodes through per-node lists (rewrite.cc reduce_tree_height: the
    nodes whose larger operand a value is), and a value combined with more than 24 earlier ones moves into a hash table.
    A late value multiplied with / added to 60 inputs, every pair twice and in both operand orders, summed in long chains
    that the reduction opens: duplicates merge, and the emulator gives the reference's witnesses for every tile width."""
    import cwc_import
    Builder = cwc_import.load().graphgen.builder.Builder
    rnd = random.Random(5)
    b = Builder()
    xs = b.input("in", 60)
    y = b.add(b.mul(xs[0], xs[1]), xs[2])          # made after every input: the larger operand of what follows
    prods = [b.mul(x, y) for x in xs] + [b.mul(y, x) for x in xs]
    sums = [b.add(y, x) for x in xs] + [b.add(x, y) for x in xs]
    acc = prods[0]
    for t in prods[1:] + sums:
        acc = b.add(acc, t)
    b.signal(acc)
    acc2 = sums[3]
    for t in sums[4:40]:
        acc2 = b.mul(acc2, t)
    b.signal(acc2)
    for t in (prods[7], prods[67], sums[9], sums[69], y):
        b.signal(t)
    data = b.to_bin()
    nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
    g = pkg.Graph(data)
    for key in (1, 2, 8, 64):
        blob = pe.Blob(g.export_blob(key))
        if key != 64:   # x * y and y * x are one node, and so are x + y and y + x (T = 64 keeps the reference's node order)
            assert blob.stats["n_op_compiled"] < len([n for n in nodes if n[0] not in ("Const", "Input")]) - 50
        for _ in range(2):
            row = [1] + [rnd.randrange(model.M) for _ in range(blob.n_inputs - 1)]
            got, st = pe.run(blob, row)
            assert st == 0 and got == model.evaluate(nodes, row, wit)


def test_library_kernels_match_the_sources(pkg):
    """The device code of the in-tree library was built from the kernel sources in the tree: the Makefile stamps the
    content hash of kernels.hip and its includes into the object (gwb_kernel_source_hash), and prints the same hash of
    the files as they are now.  (Round 3: a kernels.o newer than kernels.hip but built from an abandoned variant -- the
    source had been restored while its compile was running -- travelled to the GPU box and cost 2-9 %.)"""
    import subprocess
    csrc = os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc")
    now = subprocess.run(["make", "-s", "-C", csrc, "print-ksrc-hash"], capture_output=True, text=True, check=True).stdout.strip()
    assert len(now) == 64
    assert pkg.kernel_source_hash() == now, "libcircom_witnesscalc_amd.so holds kernels of other sources: run make"


@pytest.mark.parametrize("objname", ["kernels.o", "kernels_diag.o"])
def test_kernel_isa_uses_the_hidden_header_register_only_as_written(pkg, tmp_path, objname):
    """The interpreter's header fetch lands in XNACK_MASK_LO, a register the compiler does not know it is using
    (kernels.hip CWC_HDR_LANDING).  That is safe only while (1) nothing but the hand-written statements touches the register
    and (2) every move out of it sits right behind a full wait for scalar loads.  Checked on the ISA of the kernels as built:
    the gfx950 code object is taken out of build/kernels.o and disassembled -- a compiler bump that breaks either rule fails here."""
    llvm = "/opt/rocm/lib/llvm/bin"
    obj = os.path.join(ROOT, "circom-witnesscalc_amd", "csrc", "build", objname)  # (the diagnostic object exists once `make diag` has run: its stamped instances are compiled from the same statements)
    if not (os.path.exists(os.path.join(llvm, "llvm-objdump")) and os.path.exists(obj)):
        pytest.skip("no llvm-objdump / no %s in the tree" % objname)
    fat, co = str(tmp_path / "fatbin.bin"), str(tmp_path / "kernels_gfx950.co")
    subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj])
    subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    asm = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", "--mcpu=gfx950", co], capture_output=True, text=True, check=True).stdout.split("\n")
    assert sum("interp_kernel" in ln and ln.rstrip().endswith(">:") for ln in asm) >= 40, "interpreter instances in the disassembly"
    load = re.compile(r"\bs_load_dword xnack_mask_lo, s\[\d+:\d+\], (s\d+|0x[0-9a-f]+|\d+)\s")
    move = re.compile(r"\bs_mov_b32 s\d+, xnack_mask_lo\s")
    n_load = n_move = n_pair = 0
    for i, ln in enumerate(asm):
        if "xnack_mask" not in ln:
            continue
        m_load = load.search(ln)
        if m_load:
            n_load += 1
            # the fetch of the next header follows the move of the landed one in the same statement: the move's destination must be none of
            # the registers the load still reads (header pointer pair, offset) -- an asm output without the early-clobber mark may share them
            prev = asm[i - 1]
            mv = re.search(r"\bs_mov_b32 s(\d+), xnack_mask_lo\s", prev)
            if mv:
                base = re.search(r"xnack_mask_lo, s\[(\d+):(\d+)\], (s(\d+))?", ln)
                used = {int(base.group(1)), int(base.group(2))} | ({int(base.group(4))} if base.group(4) else set())
                assert int(mv.group(1)) not in used, "the landed header is moved into a register the next fetch reads: " + prev.strip() + " / " + ln.strip()
                n_pair += 1
            continue
        assert move.search(ln), "the compiler (or a new statement) uses xnack_mask: " + ln.strip()
        n_move += 1
        if objname != "kernels.o":  # (the stamped instances put their time stamps between the wait and the move: the product object carries rule 2)
            continue
        # walking back from the move: the wait comes before any other use of the register and before any branch
        for back in range(1, 4):
            prev = asm[i - back]
            if "s_waitcnt" in prev and "lgkmcnt(0)" in prev:
                break
            assert "xnack_mask" not in prev and not re.search(r"\bs_c?branch", prev) and prev.strip() and not prev.rstrip().endswith(":"), \
                "a move out of xnack_mask_lo without the wait in front of it: " + ln.strip()
        else:
            raise AssertionError("no s_waitcnt lgkmcnt(0) within three instructions in front of: " + ln.strip())
    assert n_move >= 100 and n_load >= n_move and n_pair >= 100


def test_multi_instruction_asm_statements_mark_their_outputs_early_clobber():
    """An asm statement of several instructions whose output is written before its last input is read needs the early-clobber mark ("=&s" /
    "=&v"), or the register allocator may give the output an input's register -- what the header fetch's statement did in one stamped instance
    (profiles/r05_header_fetch_fault.txt).  Source-level guard beside the ISA test: in the kernel sources every statement with more than one
    instruction, outputs and inputs marks every write-only output; statements of one instruction are exempt (the hardware reads before it writes)."""
    csrc = os.path.join(ROOT, "circom-witnesscalc_amd", "csrc")
    names = [n for n in os.listdir(csrc) if n.endswith((".hip", ".hpp", ".inc"))]
    checked = 0
    for name in names:
        src = open(os.path.join(csrc, name)).read()
        for m in re.finditer(r'asm\s+(?:volatile\s*)?\(', src):
            # the statement's text up to its closing parenthesis at depth 0
            i, depth = m.end(), 1
            while depth and i < len(src):
                depth += {"(": 1, ")": -1}.get(src[i], 0)
                i += 1
            stmt = src[m.end():i - 1]
            parts = re.split(r'"\s*:\s*(?=[\[":]|$)', stmt, maxsplit=1)  # template | constraints
            template = parts[0]
            if template.count("\\n") == 0:
                continue  # one instruction
            sections = re.split(r'(?<!:):(?!:)', stmt[len(template):])
            outputs = sections[1] if len(sections) > 1 else ""
            inputs = sections[2] if len(sections) > 2 else ""
            if not re.search(r'"[^"]*"\s*\(', inputs):
                continue  # no inputs to collide with
            for c in re.findall(r'"(=[^"]*)"\s*\(', outputs):
                checked += 1
                assert c.startswith("=&"), "%s: a multi-instruction asm statement with inputs has the output constraint \"%s\" without the early-clobber mark: %s" % (name, c, template[:80])
    assert checked >= 50  # (the generated multiplier / adder blocks and the header fetch)


def test_kernel_isa_has_no_per_lane_branches_in_the_interpreter_loop(pkg, tmp_path):
    """Inside the bundle loop every per-lane condition is a selection: one divergent branch in a class body makes StructurizeCFG rewrite
    the uniform branches around it into flag registers (profiles/r05_structurizer_ab.txt: the same program 10-15 % slower for code it
    never executed).  Checked on the kernels as built: an interpreter instance without divider waves holds a handful of
    s_*_saveexec (the one-lane stores of the sync / error words), its bundle loop keeps a back edge per class path, and the limb
    instances stay within reach of short branches."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    obj = os.path.join(ROOT, "circom-witnesscalc_amd", "csrc", "build", "kernels.o")
    if not (os.path.exists(os.path.join(isa_report.LLVM, "llvm-objdump")) and os.path.exists(obj)):
        pytest.skip("no llvm-objdump / no kernels.o in the tree")
    st = isa_report.instance_stats(isa_report.disassemble(obj, str(tmp_path)))
    assert len(st) >= 40
    for (T, prof, W, pack, mode), c in st.items():
        if prof:
            continue
        name = "interp_kernel<%d,%d,%d,%d,%d>" % (T, prof, W, pack, mode)
        if W == 0:
            assert c["divergent_branches"] <= 8, name + ": %d divergent branches (a per-lane `if`, `a && b` or `c ? f() : y` in the bundle loop?)" % c["divergent_branches"]
            assert c["flag_branches"] <= 12, name + ": %d flag branches (a structurized region in the bundle loop?)" % c["flag_branches"]
        else:  # (+ the divider wave's request loop, which is per-lane by nature)
            assert c["divergent_branches"] <= 60, name + ": %d divergent branches" % c["divergent_branches"]
        assert c["bytes"] < (128 << 10), name + ": %d bytes of code, beyond the reach of s_branch" % c["bytes"]


def test_slot_reuse_keeps_workspace_small(pkg):
    b = C.build_poseidon(2)
    g = pkg.Graph(b.to_bin())
    nodes, wit, _ = model.deserialize_witnesscalc_graph(b.to_bin())
    blob = pe.Blob(g.export_blob(64))
    n_values = sum(1 for n in nodes if n[0] != "Const")
    assert blob.n_slots < n_values  # liveness reuse
    # witness values stay resident (minus the ones the load-time optimiser merged or turned into constants)
    assert blob.n_slots >= len(set(wit)) - blob.stats["n_folded"] - blob.stats["n_numbered"]


def test_cli_usage(pkg):
    import subprocess
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "calc-witness")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage:" in r.stderr and "<graph.bin> <inputs.json> <witness.wtns>" in r.stderr


def test_batched_json_front_end_and_wtns_writer(pkg, tmp_path):
    """JSON array / NDJSON of input objects -> packed rows; one .wtns per set."""
    g = pkg.Graph(C.build_gadgets().to_bin())
    objs = ['{"x": "%d", "y": %d, "arr": ["1", 2, "%d", 4]}' % (7 ** k, k, 10 ** k) for k in range(5)]
    want = np.stack([g.inputs_from_json(o) for o in objs])
    assert np.array_equal(g.inputs_from_json_batch("[" + ",\n".join(objs) + "]"), want)
    assert np.array_equal(g.inputs_from_json_batch("\n".join(objs) + "\n\n"), want)
    assert g.inputs_from_json_batch("[]").shape == (0, g.n_inputs, 32)
    for bad in ('[{"x": 1}, {"x": -1}]', '[{"x": 1},]', '{"x": 1} {"x": ', '[{"nope": 1}]'):
        with pytest.raises(pkg.WitnessCalcError):
            g.inputs_from_json_batch(bad)
    # many sets: parsed on several host threads (contiguous ranges); same rows, and the LOWEST failing set is reported
    many = ['{"x": "%d", "y": %d, "arr": ["%d", 2, 3, "%d"]}' % (3 ** (k % 150), k, k * k, 2 ** (k % 250)) for k in range(700)]
    want = np.stack([g.inputs_from_json(o) for o in many])
    for threads in ("1", "3", "16"):
        os.environ["CWC_PARSE_THREADS"] = threads
        try:
            assert np.array_equal(g.inputs_from_json_batch("\n".join(many)), want)
            broken = list(many)
            broken[611] = '{"x": -5}'
            broken[305] = '{"x": "12", "y": [1, [2]]}'
            with pytest.raises(pkg.WitnessCalcError, match="input set 305"):
                g.inputs_from_json_batch("[" + ",".join(broken) + "]")
        finally:
            del os.environ["CWC_PARSE_THREADS"]
    rnd = random.Random(3)
    wit = np.frombuffer(bytes(rnd.getrandbits(8) for _ in range(3 * 4 * 32)), dtype=np.uint8).reshape(3, 4, 32)
    pkg.wtns_save_batch(wit, str(tmp_path / "w_%03lu.wtns"))
    for i in range(3):
        vals = [int.from_bytes(wit[i, k].tobytes(), "little") for k in range(4)]
        assert (tmp_path / ("w_%03d.wtns" % i)).read_bytes() == model.wtns_from_witness(vals)


def test_power_of_two_division_rewrite_is_exact(pkg):
    """Idiv/Mod by a constant 2^k are compiled as Shr/Band (rewrite.cc rewrite_pow2_divisions): same values."""
    import cwc_import
    Builder = cwc_import.load().graphgen.builder.Builder
    b = Builder()
    (x,) = b.input("x")
    ks = [0, 1, 31, 32, 33, 64, 128, 200, 253]
    for k in ks:
        b.signal(b.op("Idiv", x, b.const(1 << k)))
        b.signal(b.op("Mod", x, b.const(1 << k)))
    b.signal(b.op("Idiv", x, b.const(3)))          # not a power of two: stays a division
    b.signal(b.op("Mod", x, b.const((1 << 70) + 1)))
    g = pkg.Graph(b.to_bin())
    nodes, wit, _ = model.deserialize_witnesscalc_graph(b.to_bin())
    blob = pe.Blob(g.export_blob(4))
    classes = [pe.CLASS_NAMES[h & 0xF] for h in blob.hdr]  # noqa
    assert "BIT" in classes and "IDIVMOD" in classes
    M = model.M
    for xv in (0, 1, 5, (1 << 64) - 1, 1 << 200, M - 1, M // 2, (1 << 253) + 12345):
        assert pe.run(blob, [1, xv])[0] == model.evaluate(nodes, [1, xv], wit)


@pytest.mark.parametrize("key", [1 | STREAMS4, 2 | DIVIDER | STREAMS4, 4 | DIVIDER | STREAMS2, 8 | STREAMS2, 2 | STREAMS2])
def test_streams_split_the_independent_parts_of_a_graph(pkg, key):
    """Programs of several streams (one wavefront per stream and tile): the authV2-class graph has four large independent
    parts behind a short shared prologue.  The emulator runs every stream's bundles and checks what the kernel relies on:
    a slot is written by one stream only, a value crosses streams only from stream 0's prologue, written once, before its
    post and read behind the reader's wait; the witnesses equal the big-int oracle's."""
    b = C.build_authv2_class(scale=0.08)
    data = b.to_bin()
    nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
    g = pkg.Graph(data)
    blob = pe.Blob(g.export_blob(key))
    want_streams = 4 if key & STREAMS4 else 2
    assert blob.n_streams == want_streams and sum(1 for c in blob.stream_count[:want_streams] if c) >= 2
    assert sum(blob.stream_count[:blob.n_streams]) <= blob.n_bundles < sum(blob.stream_count[:blob.n_streams]) + 4 * blob.n_streams
    inputs = C.authv2_reference_inputs()
    rnd = random.Random(key)
    for trial in range(2):
        row = [1]
        for name, n in C.AUTHV2_INPUTS:
            row += [v if trial == 0 else rnd.randrange(model.M) for v in inputs[name][:n]] + [0] * (n - len(inputs[name][:n]))
        got, st = pe.run(blob, row)
        assert st == 0 and got == model.evaluate(nodes, row, wit)
    # fuzzed forests: independent random DAGs over every operation behind shared inputs (canonical and Montgomery values,
    # inserted conversions, divisions in several streams, sets that panic)
    for seed in range(4):
        fb = C.build_random_dag(900 + seed, n_ops=120, panic_free=(seed % 2 == 0), parts=2 + seed)
        fdata = fb.to_bin()
        fnodes, fwit, _ = model.deserialize_witnesscalc_graph(fdata)
        fblob = pe.Blob(pkg.Graph(fdata).export_blob(key))
        assert fblob.n_streams == want_streams
        for trial in range(3):
            row = [1] + [rnd.randrange(model.M) if rnd.random() < 0.6 else rnd.randrange(1 << 10) for _ in range(6)]
            got, st = pe.run(fblob, row)
            try:
                want = model.evaluate(fnodes, row, fwit)
            except model.ReferencePanic:
                assert st != 0
                continue
            assert st == 0 and got == want
    # a graph that is one piece keeps one stream
    one = pkg.Graph(C.build_sha256(64).to_bin())
    assert pe.Blob(one.export_blob(key)).n_streams == 1


@pytest.mark.parametrize("key", [2, 2 | DIVIDER, 16, 4 | GROUP, 2 | TRIPLE])
def test_compiler_rewrites_are_exact_on_chain_heavy_graphs(pkg, key):
    """Tree-height reduction, shared subexpressions, dead-node elimination, linear riders in multiplication bundles and
    request/collect divisions: long Add / Mul chains with constants, repeated operands, witness elements in the middle of
    chains and unused tails, against the big-int oracle."""
    rnd = random.Random(1000 + key)
    for case in range(4):
        b = C.build_chain_heavy(1000 * key + case)
        data = b.to_bin()
        nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
        g = pkg.Graph(data)
        blob = pe.Blob(g.export_blob(key))
        for _ in range(3):
            row = [1] + [rnd.choice([0, 1, model.M - 1, rnd.randrange(model.M)]) for _ in range(5)]
            got, st = pe.run(blob, row)
            assert st == 0 and got == model.evaluate(nodes, row, wit)


def test_loader_and_compiler_under_sanitizers(tmp_path):
    """graph.cc + knobs.cc + compile.cc + rewrite.cc + costmodel.cc + program_blob.cc + optimize.cc (loader, load-time optimiser, exact rewrites, scheduler, encoder, blob) under ASan + UBSan on generated graphs,
    a fuzzed DAG, the chain-heavy graphs and a few corrupted files (no GPU involved)."""
    import subprocess
    src = os.path.join(ROOT, "circom-witnesscalc_amd", "csrc")
    exe = str(tmp_path / "compile_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "compile_sanitize.cc"),
                           os.path.join(src, "graph.cc"), os.path.join(src, "knobs.cc"), os.path.join(src, "compile.cc"), os.path.join(src, "rewrite.cc"), os.path.join(src, "costmodel.cc"),
                           os.path.join(src, "program_blob.cc"), os.path.join(src, "optimize.cc")])
    files = []
    cases = {"gadgets": C.build_gadgets(), "poseidon3": C.build_poseidon(3), "dag": C.build_random_dag(5, n_ops=300),
             "chains": C.build_chain_heavy(3), "bigint": C.build_bigint_class(k=3, rounds=2)}
    rnd = random.Random(9)
    for name, b in cases.items():
        data = b.to_bin()
        f = tmp_path / (name + ".bin")
        f.write_bytes(data)
        files.append(str(f))
        for k in range(3):  # corrupted variants: flipped byte, truncation
            bad = bytearray(data)
            bad[rnd.randrange(14, len(bad))] ^= 1 << rnd.randrange(8)
            g = tmp_path / ("%s_bad%d.bin" % (name, k))
            g.write_bytes(bytes(bad[:len(bad) - (k * 7)]))
            files.append(str(g))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and "done rc=0" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


@pytest.mark.parametrize("perturb", [None, 1, -1])
@pytest.mark.parametrize("which", ["div_digits_test", "div_short_test", "div_recip_test", "div_3by2_test"])
def test_digitwise_division_on_host(tmp_path, perturb, which):
    """u256_divrem_digits and u128_divrem_64 (Idiv / Mod bundles) == the bit-serial division, also when the
    floating-point quotient-digit estimate is off by one in either direction; the division by an invariant limb of the
    scan bundles (reciprocal + two-by-one steps, its reciprocal made with u128_divrem_64) == unsigned __int128 division."""
    import subprocess
    exe = str(tmp_path / which)
    flags = [] if perturb is None else ["-DCWC_TEST_PERTURB_QHAT=%d" % perturb]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "native", which + ".cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and " 0 mismatches" in out.stdout, out.stdout


@pytest.mark.parametrize("constant_time", [False, True])
def test_field_inversion_on_host(tmp_path, constant_time):
    """fr_inv (safegcd divsteps, the inversion of the Div bundles) == Fermat's x^(r-2), x * inv(x) == 1, inv(0) == 0,
    with the variable-time inner loop the kernels use and with the constant-time one."""
    import subprocess
    exe = str(tmp_path / "inv_test")
    flags = ["-DCWC_CONSTANT_TIME_INVERSE"] if constant_time else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "native", "inv_test.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and " 0 mismatches" in out.stdout, out.stdout


def test_schedule_quality_guard(pkg):
    """The schedule of the bench workloads must not silently regress.  A wave's time is the sum of its bundles, priced per
    class with the cycles measured on MI355X (kCycles: compile_internal.hpp, costmodel.cc): authV2-class at T = 2 with the divider wave 30.5 M
    cycles in round 2 (narrow four-lane multiplication bundles; 33.0 M without them), sha256_512 at T = 1: 5 399 bundles."""
    g = pkg.Graph(C.build_authv2_class().to_bin())
    bl = pe.Blob(g.export_blob(2 | DIVIDER))
    cb = dict(zip(pe.CLASS_NAMES, bl.stats["class_bundles"]))
    est = bl.stream_cycles[0]  # (the compiler's own estimate: per-class cycles, less what operand forms save)
    assert est <= 30.0e6 and cb["MULQ"] + cb["MULF"] >= 2500 and cb["DIVREQ"] == cb["DIVGET"] <= 275 and cb["DIV"] == 0, (est, cb)
    bl = pe.Blob(g.export_blob(4))
    cb = dict(zip(pe.CLASS_NAMES, bl.stats["class_bundles"]))
    assert bl.n_bundles <= 27500 and cb["DIV"] <= 275
    g = pkg.Graph(C.build_sha256(512).to_bin())
    assert pe.Blob(g.export_blob(1)).n_bundles <= 5600


def test_cost_table_calibration_file(pkg, tmp_path):
    """The cost model's cycle table is read once at load time: built-in values, CWC_MODEL_CYCLES, or the calibration file
    tools/gpu_calibrate.py --write leaves behind (CWC_MODEL_CYCLES_FILE / model_cycles.txt beside the program cache).
    Entries far from the built-in value and unknown classes are ignored; the environment string wins over the file."""
    import subprocess
    f = tmp_path / "model_cycles.txt"
    f.write_text("1:2100,2:750,99:5,3:1,11:1400\n")
    code = "import sys; sys.path.insert(0, %r); import cwc_import; m = cwc_import.load().model_cycles(); print(m['MUL'], m['LIN'], m['DIV'], m['MULQ'])" % ROOT
    env = dict(os.environ)
    env.pop("CWC_MODEL_CYCLES", None)
    env.pop("CWC_MODEL_CYCLES_FILE", None)
    base = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120).stdout.split()
    assert base == ["2015.0", "706.0", "55000.0", "1306.0"], base
    got = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(env, CWC_MODEL_CYCLES_FILE=str(f)), timeout=120).stdout.split()
    assert got == ["2100.0", "750.0", "55000.0", "1400.0"], got
    got = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(env, CWC_MODEL_CYCLES_FILE=str(f), CWC_MODEL_CYCLES="1:1900"), timeout=120).stdout.split()
    assert got == ["1900.0", "706.0", "55000.0", "1306.0"], got
    # the default place: model_cycles.txt in the program cache's directory
    (tmp_path / "cache").mkdir()
    (tmp_path / "cache" / "model_cycles.txt").write_text("2:800")
    got = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(env, CWC_PROGRAM_CACHE=str(tmp_path / "cache")), timeout=120).stdout.split()
    assert got == ["2015.0", "800.0", "55000.0", "1306.0"], got


def test_reference_graph_check_tool(pkg):
    """tools/check_reference_graph.py -- the one command a maintainer with cargo runs on a reference-built `.bin` (readers
    agree, writer reproduces the bytes, witness equals the oracle's, `.wtns` equals the reference's) -- on the one pair
    of reference-derived files this repository holds: the circuit1 fixture and its hand-derived 204-byte `.wtns`."""
    import subprocess
    tool = os.path.join(ROOT, "tools", "check_reference_graph.py")
    r = subprocess.run([sys.executable, tool, os.path.join(GOLD, "circuit1.bin"), os.path.join(GOLD, "circuit1_inputs.json"), os.path.join(GOLD, "circuit1.wtns")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count("True") == 4, r.stdout + r.stderr
    other = os.path.join(os.environ.get("TMPDIR", "/tmp"), "cwc_check_tool_inputs_%d.json" % os.getpid())  # other inputs: the witness differs from the fixture's
    with open(other, "w") as f:
        f.write('{"a": ["106"], "b": ["303"]}')
    try:
        r = subprocess.run([sys.executable, tool, os.path.join(GOLD, "circuit1.bin"), other, os.path.join(GOLD, "circuit1.wtns")], capture_output=True, text=True, timeout=300)
    finally:
        os.unlink(other)
    assert r.returncode != 0 and r.stdout.count("True") == 3, r.stdout


def test_probabilistic_passes_of_the_reference(pkg, monkeypatch):
    """SURVEY 8(f) f2, second half: the reference's random-evaluation passes (src/graph.rs:499-583 random_eval /
    value_numbering / constants) as an opt-in load-time pass (CWC_RANDOM_EVAL=1).  Algebraically equal nodes of different
    shape -- (a + b) * c and a * c + b * c, sums in another association, x - x, equal-valued operands of a non-algebraic
    operation -- become one node / a constant; witnesses stay those of the reference on fuzzed graphs, panicking rows
    included (operations that can fail are random functions in the evaluation: never folded, never dropped)."""
    import cwc_import
    Builder = cwc_import.load().graphgen.builder.Builder
    b = Builder()
    a, bb, c = b.input("a")[0], b.input("b")[0], b.input("c")[0]
    e1 = b.mul(b.add(a, bb), c)
    e2 = b.add(b.mul(a, c), b.mul(bb, c))
    e3 = b.sub(b.add(a, b.add(bb, c)), b.add(b.add(c, a), bb))
    e4, e5 = b.op("Shr", e1, b.const(3)), b.op("Shr", e2, b.const(3))
    e6 = b.op("Shl", a, bb)  # can fail: stays, reports
    for x in (e1, e2, e3, e4, e5, e6):
        b.signal(x)
    data = b.to_bin()
    nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
    counts = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("CWC_RANDOM_EVAL", mode)
        blob = pe.Blob(pkg.Graph(data).export_blob(1))
        counts[mode] = blob.stats["n_op_compiled"]
        for row in ([1, 12345, 7, 777], [1, 0, 0, 0], [1, model.M - 1, 5, 2]):
            got, st = pe.run(blob, row)
            try:
                want = model.evaluate(nodes, row, wit)
            except model.ReferencePanic:
                assert st != 0
                continue
            assert st == 0 and got == want
    assert counts["1"] <= 5 < 12 <= counts["0"], counts  # (a + b) * c, one Shr, the Shl and little else
    monkeypatch.setenv("CWC_RANDOM_EVAL", "1")
    rnd = random.Random(21)
    for s_ in range(10):
        bld = C.build_random_dag(100 + s_, n_ops=260, panic_free=(s_ % 2 == 0), parts=1 + s_ % 3) if s_ < 7 else C.build_chain_heavy(s_, n_chains=14)
        data = bld.to_bin()
        nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
        g = pkg.Graph(data)
        for key in (1, 4, 2 | DIVIDER):
            blob = pe.Blob(g.export_blob(key))
            for _ in range(2):
                row = [1] + [rnd.randrange(model.M) if rnd.random() < 0.6 else rnd.randrange(1 << 10) for _ in range(blob.n_inputs - 1)]
                got, st = pe.run(blob, row)
                try:
                    want = model.evaluate(nodes, row, wit)
                except model.ReferencePanic:
                    assert st != 0
                    continue
                assert st == 0 and got == want, (s_, key)


def fold_heavy_builder(variant, rnd):
    """A graph built to fold: every operator on CONSTANT operands over a grid of edge values (variant 0 keeps the ones the
    reference panics on), same-operand forms, field identities, duplicated subexpressions, dead code (also fallible dead
    code).  Shared by the emulator test below and the GPU on / off test of the load-time optimiser."""
    import cwc_import
    Builder = cwc_import.load().graphgen.builder.Builder
    M = model.M
    edge = [0, 1, 2, 5, 253, 254, 255, M - 1, M - 2, M // 2, M // 2 + 1, 1 << 253, (1 << 64) - 1, M & ((1 << 253) - 1), M ^ (M & ((1 << 253) - 1))]
    duo = ["Mul", "Div", "Add", "Sub", "Idiv", "Mod", "Eq", "Neq", "Lt", "Gt", "Leq", "Geq", "Land", "Lor", "Shl", "Shr", "Bor", "Band", "Bxor"]
    b = Builder(dedup_consts=(variant % 2 == 0))
    x, y = b.input("x")[0], b.input("y")[0]
    outs = []
    pairs = [(rnd.choice(edge), rnd.choice(edge)) for _ in range(40)]
    for op in duo:
        for va, vb in pairs[:12 if variant else 40]:
            if variant:  # variants 1..3: only constant operations the reference can evaluate (their VALUES are compared);
                try:     # variant 0 keeps the ones that panic there: they must survive the pass and report on every row
                    model.eval_duo(op, va, vb)
                except model.ReferencePanic:
                    continue
            outs.append(b.op(op, b.const(va), b.const(vb)))
        outs.append(b.op(op, x, x))                                     # same operand
        outs.append(b.op(op, x, b.const(0)))
        outs.append(b.op(op, b.const(0), x))
        outs.append(b.op(op, x, b.const(1)))
        outs.append(b.op(op, b.const(1), y))
        outs.append(b.op(op, b.op(op, x, y), b.op(op, x, y)))         # duplicated subexpression
        outs.append(b.op(op, b.op("Add", x, y), b.op("Add", y, x)))     # ... up to commutation
    for v in edge[:6]:
        outs.append(b.neg(b.const(v)))
        outs.append(b.tern(b.const(v), x, y))
        outs.append(b.tern(x, b.const(v), b.const(v)))
    dead = b.mul(b.add(x, y), b.const(77))                              # unused: shaken
    dead_fallible = b.op("Shl", x, y)                                   # unused but can fail: kept, still reports
    assert dead and dead_fallible
    for o in outs[::2] if variant == 3 else outs:
        b.signal(o)
    return b


def test_load_time_optimiser_is_exact(pkg):
    """SURVEY 8(f) f2 (optimize.cc; the reference's build-time passes src/graph.rs:358-619 as exact load-time rewrites):
    every operator applied to CONSTANT operands over a grid of edge values -- folded with eval_fr semantics unless the
    reference would panic, in which case the node must survive and still report --, same-operand comparisons, the field
    identities, duplicated subexpressions and dead code.  The optimised program (emulated) against the big-int model on
    the graph as written, with and without the pass."""
    M = model.M
    rnd = random.Random(12)
    for variant in range(4):
        b = fold_heavy_builder(variant, rnd)
        data = b.to_bin()
        nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
        compared = 0
        for env in ({}, {"CWC_NO_LOAD_OPTIMIZE": "1"}):
            os.environ.update(env)
            try:
                g = pkg.Graph(data)
                blobs = [pe.Blob(g.export_blob(k)) for k in (1, 4, 64)]
            finally:
                for k in env:
                    del os.environ[k]
            if not env:
                assert blobs[0].stats["n_folded"] > 100 and blobs[0].stats["n_numbered"] > 10 and blobs[0].stats["n_shaken"] >= 1
            else:
                assert blobs[0].stats["n_folded"] == 0
            for row in ([1, 0, 0], [1, 5, 5], [1, M - 1, 3], [1, rnd.randrange(M), rnd.randrange(M)], [1, 1 << 200, 2], [1, 3, 200]):
                try:
                    want = model.evaluate(nodes, row, wit)
                    panic = False
                except model.ReferencePanic:
                    panic = True
                compared += not panic
                for blob in blobs:
                    got, st = pe.run(blob, row)
                    assert (st != 0) == panic, (variant, row)
                    if not panic:
                        assert got == want, (variant, row)
        assert (compared == 0) if variant == 0 else (compared >= 6), (variant, compared)


def test_cost_model_program_choice_is_host_only_and_sane(pkg):
    """gwb_graph_pick_tile_width needs no device (rank 0 of a multi-GPU job asks it before exporting the program), sees the
    divisions of the graph as loaded (a divider-wave program while every pair is resident, none for a graph without
    divisions) and widens the tile with the batch."""
    g = pkg.Graph(C.build_authv2_class(scale=0.3).to_bin())
    keys = {b: g.pick_tile_width(b) for b in (1, 256, 1024, 4096, 16384, 65536)}
    assert keys[1024] & 0x700 and keys[256] & 0x700, keys          # divider programs at small batches
    assert not keys[65536] & 0x700 and (keys[65536] & 0xff) >= 16, keys
    widths = [keys[b] & 0xff for b in sorted(keys)]
    assert widths == sorted(widths), keys
    s = pkg.Graph(C.build_sha256(512).to_bin())
    assert not s.pick_tile_width(1024) & 0x700 and not s.pick_tile_width(4096) & 0x700
