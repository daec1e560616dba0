"""The pack schedule (csrc/pack_schedule.cc, gwb_pack_schedule): which witness rows the divider wave of a program may convert and
store between its division requests.  Host only; every property is recomputed here from the exported program."""
import numpy as np
import pytest

import cwc_import
C = cwc_import.load().graphgen.circuits
import program_emulator as pe

DIVIDER, GROUP, STREAMS2 = 0x100, 0x200, 0x800
C_DIVREQ, CTRL_ACTIVE, CTRL_MASK = 9, 8, 15
REF_CONST, REF_CANON = 0x80000000, 0x40000000


def _producers(blob):
    """(last bundle with an ACTIVE record whose destination is the slot, per value slot; bundles of the requests)"""
    G, T = blob.G, blob.T
    slot_bytes, first = 32 * T, blob.n_const * 32 * T
    recs = np.asarray(blob.recs, dtype=np.uint64).reshape(blob.n_bundles, G, 4)
    dctl = recs[:, :, 2]
    dst = dctl & np.uint64(0xFFFFFFFF & ~CTRL_MASK)
    active = (dctl & np.uint64(CTRL_ACTIVE)) != 0
    inside = active & (dst >= first) & (dst < first + blob.n_slots * slot_bytes)
    producer = np.full(blob.n_slots, -1, dtype=np.int64)
    b_idx, _ = np.nonzero(inside)
    slots = ((dst[inside] - np.uint64(first)) // np.uint64(slot_bytes)).astype(np.int64)
    np.maximum.at(producer, slots, b_idx)
    req = np.nonzero((np.asarray(blob.hdr, dtype=np.uint64) & np.uint64(15)) == C_DIVREQ)[0]
    return producer, req


def _check_schedule(g, key):
    blob = pe.Blob(g.export_blob(key))
    order, ready, n_inline = g.pack_schedule(key)
    nw = blob.n_witness
    assert order.size == nw and np.array_equal(np.sort(order), np.arange(nw))
    producer, req = _producers(blob)
    assert ready.size == len(req) + 1
    assert (np.diff(ready.astype(np.int64)) >= 0).all() and ready[-1] <= nw
    assert n_inline <= ready[-1]
    refs = np.asarray(blob.witness_refs, dtype=np.uint64)
    for k in range(ready.size):
        # the lag rule: with k posts seen (the newest one is request k - 1's), only what request k - 2 has in front of it
        ent = order[: ready[k]]
        r = refs[ent]
        slots = (r[(r & np.uint64(REF_CONST)) == 0] & np.uint64(~REF_CANON & 0xFFFFFFFF)).astype(np.int64)
        if slots.size == 0:
            continue
        assert k >= 2, "a computed row counted ready before two posts"
        assert (producer[slots] >= 0).all() and (producer[slots] < req[k - 2]).all(), (hex(key), k)
    return blob, order, ready, n_inline


@pytest.mark.parametrize("key", [1 | DIVIDER, 2 | DIVIDER, 4 | DIVIDER])
def test_gadget_graph_schedule(pkg, key):
    g = pkg.Graph(C.build_gadgets().to_bin())
    blob, order, ready, n_inline = _check_schedule(g, key)
    assert blob.divider == 1 and ready.size > 1 and ready[-1] > 0
    # the same program through export -> import gets the same schedule
    o2, r2, n2 = pkg.pack_schedule_of_blob(g.export_blob(key))
    assert np.array_equal(order, o2) and np.array_equal(ready, r2) and n_inline == n2


@pytest.mark.parametrize("key", [1 | DIVIDER, 2 | DIVIDER, 4 | DIVIDER])
def test_graph_without_divisions_packs_nothing_inline(pkg, key):
    g = pkg.Graph(C.build_poseidon(2).to_bin())
    _, order, ready, n_inline = _check_schedule(g, key)
    assert n_inline == 0 and ready[-1] == 0


@pytest.mark.parametrize("key", [2, 2 | GROUP, 2 | DIVIDER | STREAMS2])
def test_programs_out_of_scope_pack_nothing_inline(pkg, key):
    g = pkg.Graph(C.build_gadgets().to_bin())
    order, ready, n_inline = g.pack_schedule(key)
    assert n_inline == 0 and not ready.any() and np.array_equal(order, np.arange(order.size))


@pytest.mark.parametrize("key", [1 | DIVIDER, 2 | DIVIDER, 4 | DIVIDER])
def test_authv2_class_schedule(pkg, key):
    g = pkg.Graph(C.build_authv2_class().to_bin())
    blob, order, ready, n_inline = _check_schedule(g, key)
    if key == 2 | DIVIDER:  # what the cost model picks for 1024 sets: at most 2 % of the rows are produced behind the last request
        assert blob.n_witness - int(ready[-1]) <= 0.02 * blob.n_witness
        assert n_inline > 0
