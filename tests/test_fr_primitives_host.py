"""The vectors of tests/fr_vectors.py do what they claim (CPU; the GPU side is tests/test_gpu_fr_primitives.py).

The lane-cooperative sequences resolve carries between lanes with one scalar addition over generate / propagate masks,
carries = ((G | P) + G) ^ P, and the subtraction of r the same way.  Random operands set a propagate bit together with a
carry-in or borrow-in about once in 2^64 lanes, so the P terms, the exclusion of the top lanes and SEL = G | B1 with the
deciding borrow arriving through a propagating lane are dead code for every random test.  Here the generator's emulator
(tools/codegen/gen_fr_mul_coop.py: the instruction list that is printed, executed on 64 lanes) observes the masks, and the
vector sets are required to reach those states in numbers, in every group position of the wave, beside idle and beside
eventful neighbours."""
import os
import subprocess

import pytest

import fr_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "circom-witnesscalc_amd", "csrc")
gen = V.gen


def _required(seq):
    req = [(c, k) for c in V.EVENTS for k in V.SEQ_KINDS[seq]]
    for k in V.SEQ_KINDS[seq]:
        req += [(c, k) for c in V.RIDER_CLASSES.get(k, ())]
    return req


@pytest.mark.parametrize("seq", ["mul", "mulr", "lin"])
def test_cooperative_vectors_reach_the_carry_and_borrow_states(seq):
    """Counted by the emulator, per sequence and per kind of group (product / add / subtract): at least 16 group operations
    of every class of fr_vectors.EVENTS and of the rider list, each class in each of the 16 group positions once between
    idle groups and once between groups that show a carry / borrow event themselves; every emulated result equals plain
    Python.  (The issue asks for the counts per sequence; per kind is stricter: in fr_mul_coop4r the product groups reach
    the states as well as the riders beside them.)

    Two adjacent propagating lanes with a carry coming in cannot happen in the CARRY pass at K = 4, for any operands.  The
    first pass adds the previous lane's overflow to every lane.  Lane 0 receives the top lane's overflow, which is zero (a
    product is below 2r < 2^255; a rider's top overflow is cleared: that is where a subtraction's 2^256 leaves), so lane 0
    never generates and the carry into lane 1 is always zero: lane 1 cannot have P with a carry-in.  Lane 3 is the top
    lane and is kept out of P.  That leaves lane 2 alone (P_2 with the carry lane 1 generated), so the class "two adjacent"
    does not exist for the carry pass and the carry class is always lane 2: the test asserts exactly that.  In the borrow
    pass lane 0 does generate (W_0 < r_0) and lanes 1 and 2 can both propagate: class borrow2."""
    d = V.build(seq)
    waves, quiet = d["waves"], d["quiet"]
    results, counts, cover = V.census(seq, waves, quiet)
    for ops, res in zip(waves, results):
        for op, got in zip(ops, res):
            assert got == V.want(*op), (seq, op, got)
    for key in _required(seq):
        assert counts.get(key, 0) >= 16, (seq, key, counts.get(key, 0))
        for mode in ("quiet", "loud"):
            assert cover.get(key + (mode,), set()) == set(range(16)), (seq, key, mode, sorted(cover.get(key + (mode,), ())))
    # the operand limits of the header: a anywhere below 2^256 for a product, b below r
    if V.MUL in V.SEQ_KINDS[seq]:
        a_all = {op[0] for ops in waves for op in ops if op[2] == V.MUL}
        assert {V.R, V.R + 1, V.B256 - 1} <= a_all
    assert all(op[1] < V.R and (op[2] == V.MUL or op[0] < V.R) for ops in waves for op in ops)
    # sub patterns across the 16 groups of a wave (rider sequences)
    if V.ADD in V.SEQ_KINDS[seq]:
        pats = {tuple(op[2] for op in ops) for i, ops in enumerate(waves) if i not in quiet}
        assert (V.ADD,) * 16 in pats and (V.SUB,) * 16 in pats and (V.ADD, V.SUB) * 8 in pats and (V.SUB, V.ADD) * 8 in pats
        assert len(pats) >= 10
        if seq == "mulr":
            assert any(len(set(p)) == 3 for p in pats)   # products mixed in


@pytest.mark.parametrize("seq", ["mul", "mulr", "lin"])
def test_carry_pass_event_is_always_lane_2(seq):
    emu = V.Coop4(seq)
    for ops in V.build(seq)["waves"]:
        st_masks = {}
        orig = [emu.p.ins[i].fn for i in emu.xor]

        def spy(st, f=orig[0]):
            p = st.s["%[sp]"]
            f(st)
            st_masks["hit"] = p & st.s[emu.X]
        emu.p.ins[emu.xor[0]].fn = spy
        emu.run(ops)
        emu.p.ins[emu.xor[0]].fn = orig[0]
        assert st_masks["hit"] & ~0x4444444444444444 == 0


APPLIES = {"mul": ("carry_p_zero", "borrow_p_zero", "top_kept", "sel_first_only"), "mulr": V.MUTANTS, "lin": V.MUTANTS}


@pytest.mark.parametrize("seq", ["mul", "mulr", "lin"])
def test_mutants_of_the_resolution_are_caught(seq):
    """Every mutant gives a wrong result on the vectors of every sequence it applies to; the mask mutants (P terms, SEL) on
    groups of every kind the sequence has, so in fr_mul_coop4r on a product group too.

    What each mutant does to the emitted sequence, and whether the generator's own check(4, rounds=400) notices (measured when
    this test was written; nothing below asserts it):
      carry_p_zero    P of the carry resolution forced to zero: a carry into an all-ones lane stops there.
                      check: misses it for the plain product, catches it for the rider sequences (their edge list, round 1).
      borrow_p_zero   P of the borrow resolution forced to zero.  check: as above (product missed, riders caught).
      top_kept        the four `s_andn2 ..., top` removed: a top lane's borrow runs into the next group.  check: caught everywhere
                      (any group with W < r beside a group with W >= r).
      top_kept_carry  only the two of the carry pass removed.  No effect on the plain product (its top lane never generates or
                      propagates: the value is below 2^255), so it is no mutant there; the riders' subtractions carry their 2^256
                      out of the top lane.  check: caught for the rider sequences.
      sel_first_only  SEL = B1 instead of G | B1: a value below r by a borrow that arrived late is taken for >= r.
                      check: misses it for the plain product, catches it for the rider sequences."""
    waves = V.build(seq)["waves"]
    for m in V.MUTANTS:
        emu = V.Coop4(seq, m)
        wrong = {}
        per_kind = m in ("carry_p_zero", "borrow_p_zero", "sel_first_only")
        for ops in waves:
            if m in APPLIES[seq] and wrong and (not per_kind or set(wrong) == set(V.SEQ_KINDS[seq])):
                break   # caught
            res, _ = emu.run(ops)
            for op, got in zip(ops, res):
                if got != V.want(*op):
                    wrong[op[2]] = wrong.get(op[2], 0) + 1
        if m not in APPLIES[seq]:
            assert not wrong, (seq, m)   # equivalent there (see the table above)
            continue
        assert wrong, (seq, m)
        if per_kind:
            assert set(wrong) == set(V.SEQ_KINDS[seq]), (seq, m, wrong)


def test_cooperative_generator_reproduces_the_committed_inc(tmp_path):
    for K, riders, lin_only in ((4, False, False), (4, True, False), (4, True, True), (8, False, False), (2, False, False)):
        name = "fr_addsub_coop%d_gfx950.inc" % K if lin_only else "fr_mul_coop%d%s_gfx950.inc" % (K, "r" if riders else "")
        out = tmp_path / name
        gen.emit(K, str(out), riders=riders, lin_only=lin_only)
        assert out.read_bytes() == open(os.path.join(CSRC, name), "rb").read(), name


@pytest.mark.parametrize("mod", [V.R, V.Q], ids=["r", "q"])
def test_one_lane_vectors_hold_the_chosen_values(mod):
    """The one-lane products are chosen by u = (a b + m mod) / 2^256, the value in front of the conditional subtraction.
    u = 2 mod - 1 is unreachable: 2^256 u = a b + m mod <= (2^256 - 1)(mod - 1) + (2^256 - 1) mod < 2^256 (2 mod - 1)."""
    pairs, stats = V.one_lane_mul(mod)
    us = {V.mont_u(a, b, mod) for a, b in pairs}
    assert {0, 1, mod - 1, mod, mod + 1} <= us and 2 * mod - 1 not in us
    assert max(us) < 2 * mod - 1
    for k in range(1, 8):   # a borrow that runs through exactly k words of u - mod, both ways it can end
        low = (1 << (32 * k)) - 1
        hit = [u for u in us if u & low == mod & low and (u >> (32 * k)) & V.M32 != (mod >> (32 * k)) & V.M32]
        assert any(u < mod for u in hit) and any(u > mod for u in hit), k
        assert stats["u=r in %d low words" % k] >= 2
    res = {a * b * pow(V.B256, -1, mod) % mod for a, b in pairs}
    for i in range(8):
        for v in (0, V.M32):
            if i == 7 and v:
                continue   # the modulus' top word is 0x30644e72
            assert any((t >> (32 * i)) & V.M32 == v for t in res if t), (i, v)
            for side in ((p[0] for p in pairs), (p[1] for p in pairs)):
                assert any((x >> (32 * i)) & V.M32 == v for x in side), (i, v)
        assert any((p[0] >> (32 * i)) & V.M32 == 1 for p in pairs) and any((p[1] >> (32 * i)) & V.M32 == 1 for p in pairs)
    assert {mod, mod + 1, V.B256 - 1} <= {a for a, _ in pairs}
    sums = {a + b for a, b in V.one_lane_addsub(mod)}
    diffs = {a - b for a, b in V.one_lane_addsub(mod)}
    assert {0, 1, mod - 1, mod, mod + 1, 2 * mod - 2} <= sums and {0, 1, -1, mod - 1, 1 - mod} <= diffs
    for k in range(1, 8):
        w = 1 << (32 * k)
        assert {w - 1, w, w + 1} <= sums and {w - 1, w, w + 1, -w, 1 - w, -1 - w} <= diffs


def test_device_harness_compiles_for_gfx950(tmp_path):
    """compile only (no GPU here): the harness of tests/test_gpu_fr_primitives.py must not arrive uncompilable"""
    src = os.path.join(ROOT, "tests", "native", "fr_primitives.hip")
    p = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + CSRC,
                        "-I" + os.path.join(ROOT, "circom-witnesscalc_amd", "r1cs"), src, "-o", str(tmp_path / "fr_primitives")],
                       capture_output=True, text=True, timeout=1800)
    assert p.returncode == 0, p.stderr[-4000:]


DIVIDER, STREAMS2 = 0x100, 0x800   # GWB_TILE_ASYNC_DIVIDER, GWB_TILE_STREAMS2
INTERPRETER_KEYS = (1, 2, 4, 2 | DIVIDER, 2 | DIVIDER | STREAMS2)
INTERPRETER_CASES = [("mul", 4), ("mul", 16), ("riders", 2), ("riders", 4), ("fused0", 4), ("fused1", 4), ("fused2", 4), ("fused3", 4)]


def interpreter_case(pkg, shape, n, key):
    """-> (graph bytes, rows, blob, names of the narrow classes the program must have) or None where the case does not apply:
    16 products fill a narrow bundle at tile width 1 only, fused bundles exist at tile widths 1 and 2 (program_dev.h)."""
    import program_emulator as pe
    if n == 16 and key != 1:
        return None
    data = V.interpreter_graph(pkg.graphgen.builder.Builder, shape, n).to_bin()
    blob = pe.Blob(pkg.Graph(data).export_blob(key))
    cb = dict(zip(pe.CLASS_NAMES, blob.stats["class_bundles"]))
    need = "MULF" if shape.startswith("fused") and (key & 0xff) <= 2 else "MULQ"
    assert cb[need] > 0 and cb["MUL"] == 0, (shape, n, hex(key), cb)   # not fr_mul_wave instead
    return data, V.interpreter_rows(shape, n), blob, need


def test_interpreter_programs_receive_the_events(pkg, monkeypatch):
    """tests/test_gpu_fr_primitives.py pushes these rows through calc_witness_batch.  Here, without a GPU: the compiled programs
    hold narrow bundles (MULQ, with riders; MULF) at every tile key used, the program emulator gives the reference's witnesses,
    and the operand words it sees at those bundles -- in the order the compiler chose to pass them -- show every event class
    on the lane emulators: the states are reached inside the interpreter, not only in the harness."""
    import program_emulator as pe
    from oracle import model
    monkeypatch.setenv("CWC_FUSE", "1001")
    for shape, n in INTERPRETER_CASES:
        for key in INTERPRETER_KEYS:
            case = interpreter_case(pkg, shape, n, key)
            if case is None:
                continue
            data, rows, blob, need = case
            nodes, wit, _ = model.deserialize_witnesscalc_graph(data)
            wits, counts, n_fused = V.interpreter_census(pe, blob, rows)
            assert all(w == model.evaluate(nodes, row, wit) for w, row in zip(wits, rows))
            for c in V.EVENTS:
                assert counts.get((c, V.MUL), 0) >= 1, (shape, n, hex(key), c)
            if shape == "riders" and (key & 0xff) <= 2:   # (at tile width 4 the linear nodes get a bundle of their own)
                for c in V.EVENTS:
                    assert counts.get((c, V.ADD), 0) >= 1 and counts.get((c, V.SUB), 0) >= 1, (shape, n, hex(key), c)
            if need == "MULF":
                assert n_fused >= len(rows)
                lin = V.SUB if shape in ("fused1", "fused2") else V.ADD   # (of (x y + z) - w the compiler fuses x y + z)
                for c in V.EVENTS[1:]:   # (the later stages are solved for borrow-pass targets)
                    assert counts.get((c, lin), 0) >= 1, (shape, n, hex(key), c)
