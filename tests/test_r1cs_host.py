"""The `.r1cs` loader of libcwc_r1cs.so (include/graph_witness_r1cs.h) against the independent Python writer, its refusals,
a mutation fuzz, the Python checker against honest oracle witnesses, and the check-witness CLI's usage errors.  CPU only."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import cwc_import
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
C = PKG.graphgen.circuits
CLI = os.path.join(os.path.dirname(PKG.R1CS_LIB_PATH), "check-witness")

# x0 * x1 = x2 over wires [1, x0, x1, x2, x3]; a linear one x3 = 5 * x0 - x1 + 7; one with -1 / +1 / general coefficients
CONS = [({1: 1}, {2: 1}, {3: 1}),
        ({}, {}, {4: 1, 1: F.R - 5, 2: 1, 0: F.R - 7}),
        ({1: 3, 2: F.R - 1}, {0: 1}, {1: 3, 2: F.R - 1})]


def _load(data):
    return PKG.R1cs(data)


def test_round_trip_info(pkg):
    for order in ((1, 2, 3), (3, 1, 2), (2, 3, 1)):
        r = _load(F.write_r1cs(5, CONS, n_pub_out=1, n_pub_in=1, n_prv_in=2, order=order))
        assert r.info == {"n_wires": 5, "n_pub_out": 1, "n_pub_in": 1, "n_prv_in": 2, "n_constraints": 3, "n_labels": 5,
                          "n_factors_a": 3, "n_factors_b": 2, "n_factors_c": 7}, (order, r.info)
    # a derived circuit: the counts are what the writer wrote
    b = _poseidon_builder()
    cons = F.derive_r1cs(b)
    r = _load(F.write_r1cs(len(b._witness), cons))
    assert r.info["n_constraints"] == len(cons) and r.info["n_wires"] == len(b._witness)
    assert r.info["n_factors_a"] == sum(len(a) for a, _, _ in cons) and r.info["n_factors_c"] == sum(len(c) for _, _, c in cons)
    # an unknown section type is skipped; an empty constraint system loads
    r = _load(F.container([(1, F.header_section(2, n_constraints=0)), (9, b"xyz"), (2, b""), (3, F.map_section(2))]))
    assert r.info["n_constraints"] == 0


def _rejects(data, pattern):
    with pytest.raises(PKG.WitnessCalcError, match=pattern):
        _load(data)


def test_rejections(pkg):
    good_h, good_c, good_m = F.header_section(5, n_constraints=3), F.constraints_section(CONS), F.map_section(5)
    base = [(1, good_h), (2, good_c), (3, good_m)]
    _rejects(b"r1cz" + F.write_r1cs(5, CONS)[4:], "bad magic")
    _rejects(b"r1", "truncated file header")
    _rejects(F.container(base, version=2), "unsupported version 2")
    for t in (1, 2, 3):
        _rejects(F.container([s for s in base if s[0] != t]), "missing section %d" % t)
        _rejects(F.container(base + [s for s in base if s[0] == t]), "duplicate section %d" % t)
    _rejects(F.container([(1, F.header_section(5, n_constraints=3, n8=48, prime=F.R))] + base[1:]), "n8 = 48")
    _rejects(F.container([(1, F.header_section(5, n_constraints=3, prime=F.R + 2))] + base[1:]), "prime is not BN254")
    _rejects(F.container([(1, F.header_section(5, n_constraints=3, prime=(1 << 255) - 19))] + base[1:]), "prime is not BN254")
    # truncated: the file ends inside a section, a section ends inside a record, a section is longer than its contents
    whole = F.container(base)
    _rejects(whole[:-5], "truncated section 3")
    _rejects(whole[:30], "truncated")
    _rejects(F.container([(1, good_h), (2, good_c[:-10]), (3, good_m)]), "truncated constraints section")
    _rejects(F.container([(1, good_h), (2, good_c + b"\0" * 4), (3, good_m)]), "constraints section size .* disagrees")
    _rejects(F.container([(1, good_h + b"\0"), (2, good_c), (3, good_m)]), "header section size .* disagrees")
    _rejects(F.container([(1, good_h[:-2]), (2, good_c), (3, good_m)]), "truncated header section")
    _rejects(F.container([(1, good_h), (2, good_c), (3, good_m[:-8])]), "wire-to-label map section size .* disagrees")
    _rejects(F.container([(1, good_h), (2, good_c), (3, F.map_section(5, [0, 1, 2, 3, 99]))]), "maps to label 99")
    _rejects(whole + b"\0", "trailing bytes")
    # declared counts that cannot fit: overflow-prone products
    _rejects(F.container([(1, F.header_section(5, n_constraints=0xFFFFFFF0)), (2, good_c), (3, good_m)]), "truncated constraints section")
    huge = struct.pack("<I", 0xFFFFFFFF) + good_c[4:]
    _rejects(F.container([(1, good_h), (2, huge), (3, good_m)]), "declares 4294967295 factors")
    _rejects(F.container([(1, good_h), (2, good_c), (3, good_m)])[:12] + struct.pack("<IQ", 1, 1 << 63), "truncated section 1")
    # wire and coefficient range
    _rejects(F.write_r1cs(5, [({5: 1}, {}, {})]), "references wire 5 >= nWires = 5")
    bad_coef = F.constraints_section([({1: 1}, {}, {})])
    bad_coef = bad_coef[:8] + F.R.to_bytes(32, "little") + bad_coef[40:]
    _rejects(F.container([(1, F.header_section(5, n_constraints=1)), (2, bad_coef), (3, good_m)]), "coefficient >= r")
    # custom gates (circom --O2 ... custom_templates)
    _rejects(F.container(base + [(4, b"\0" * 4)]), "custom gates .*section 4")
    _rejects(F.container(base + [(5, b"\0" * 4)]), "custom gates .*section 5")
    _rejects(F.container([(1, F.header_section(5, n_pub_out=3, n_pub_in=2, n_constraints=3)), (2, good_c), (3, good_m)]), "exceeds nWires")


def _mutations(data, rnd, n):
    for _ in range(n):
        d = bytearray(data)
        kind = rnd.randrange(6)
        if kind == 0:
            for _ in range(rnd.randrange(1, 8)):
                d[rnd.randrange(len(d))] = rnd.randrange(256)
        elif kind == 1:
            d = d[:rnd.randrange(len(d))]
        elif kind == 2:  # a length / count / wire word set to an extreme
            p = rnd.randrange(0, len(d) - 4) & ~3
            d[p:p + 4] = struct.pack("<I", rnd.choice([0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 1 << 30, 0, len(d)]))
        elif kind == 3:  # a section size lies
            p = 16  # (the first section's)
            d[p:p + 8] = struct.pack("<Q", rnd.choice([1 << 63, (1 << 64) - 1, len(d), 0, 1 << 32]))
        elif kind == 4:
            p = rnd.randrange(len(d))
            d[p:p] = bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 40)))
        else:
            for _ in range(20):
                d[rnd.randrange(12, len(d))] |= 0x80
        yield bytes(d)


def test_mutated_files_never_crash(pkg):
    rnd = random.Random(1234)
    ok = bad = 0
    bases = [F.write_r1cs(5, CONS, order=(2, 1, 3)), F.write_r1cs(5, CONS * 7)]
    for base in bases:
        for m in _mutations(base, rnd, 2000):
            try:
                r = _load(m)
                assert r.info["n_wires"] >= 1
                ok += 1
            except PKG.WitnessCalcError:
                bad += 1
    assert ok + bad == 4000 and bad > 2000, (ok, bad)


# -- the Python checker on honest witnesses of the C oracle ---------------------------------------------------------------------
def _poseidon_builder(n=2):
    b = PKG.graphgen.builder.Builder()
    ins = b.input("inputs", n)
    for h in ins:
        b.signal(h)
    b.signal(C.poseidon(b, ins, signals=True, circomlib=True))
    return b


def test_checker_on_oracle_witnesses(oracle_c):
    from tools.synth import synth_inputs
    with F.gadget_constraints():
        b = C.build_gadgets()
    for builder in (_poseidon_builder(), b):
        cons = F.derive_r1cs(builder)
        assert len(cons) > 10
        og = oracle_c.Graph(builder.to_bin())
        wit, st = og.evaluate_batch(synth_inputs("field", og.n_inputs, 3, 11))
        for s in range(3):
            if st[s]:
                continue
            w = F.row_ints(wit[s])
            assert F.check(cons, w) == (0xFFFFFFFF, 0)
            j = max(range(1, len(w)), key=lambda i: sum(i in a or i in bb or i in c for a, bb, c in cons))
            w[j] = (w[j] + 1) % F.R
            first, n = F.check(cons, w)
            assert n >= 1 and first < len(cons)


def test_checker_gadget_constraints_hold(oracle_c):
    """Num2Bits and IsZero constraints are emitted, and hold on the oracle's witness (the authV2-class graph at full size: a
    scaled-down one takes Num2Bits of fewer bits than its values have, which a real circuit would reject)."""
    from tools.synth import synth_inputs
    with F.gadget_constraints():
        b = C.build_authv2_class()
    kinds = {g[0] for g in b._r1cs_gadgets}
    assert kinds == {"num2bits", "is_zero"}
    cons = F.derive_r1cs(b)
    assert max(len(a) + len(bb) + len(c) for a, bb, c in cons) > 25  # a Num2Bits sum
    og = oracle_c.Graph(b.to_bin())
    wit, st = og.evaluate_batch(synth_inputs("field", og.n_inputs, 1, 3))
    assert not st.any()
    for s in range(1):
        assert F.check(cons, F.row_ints(wit[s])) == (0xFFFFFFFF, 0)


def test_check_arguments_are_validated_before_the_device(pkg):
    r = _load(F.write_r1cs(5, CONS))
    with pytest.raises(PKG.WitnessCalcError, match="the witness has 4 elements, the circuit 5 wires"):
        r.check_batch(np.zeros((2, 4, 32), dtype=np.uint8))
    w = bytes(PKG.wtns_from_witness([1, 2, 3]))
    with pytest.raises(PKG.WitnessCalcError, match="the witness has 3 elements"):
        r.check_wtns(w)
    with pytest.raises(PKG.WitnessCalcError, match="bad magic"):
        r.check_wtns(b"wtnx" + w[4:])
    with pytest.raises(PKG.WitnessCalcError, match="trailing bytes"):
        r.check_wtns(w + b"\0")
    with pytest.raises(PKG.WitnessCalcError, match="truncated"):
        r.check_wtns(w[:-1])
    big = bytearray(PKG.wtns_from_witness([1, 2, 3, 4, 5]))
    big[-32:] = F.R.to_bytes(32, "little")
    with pytest.raises(PKG.WitnessCalcError, match="witness element 4 is not below r"):
        r.check_wtns(bytes(big))
    with pytest.raises(PKG.WitnessCalcError, match="tile width"):
        r.set_tile_width(3)


def test_check_witness_cli_usage_errors(pkg, tmp_path):
    assert os.path.exists(CLI)
    p = subprocess.run([CLI], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr
    p = subprocess.run([CLI, "a"], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr
    p = subprocess.run([CLI, str(tmp_path / "missing.r1cs"), str(tmp_path / "missing.wtns")], capture_output=True, text=True)
    assert p.returncode == 2 and "cannot read" in p.stderr
    (tmp_path / "c.r1cs").write_bytes(F.write_r1cs(5, CONS))
    (tmp_path / "bad.r1cs").write_bytes(F.container([(1, F.header_section(5)), (2, b""), (3, F.map_section(5)), (4, b"")]))
    (tmp_path / "w.wtns").write_bytes(PKG.wtns_from_witness([1, 2, 3]))
    p = subprocess.run([CLI, str(tmp_path / "bad.r1cs"), str(tmp_path / "w.wtns")], capture_output=True, text=True)
    assert p.returncode == 2 and "custom gates" in p.stderr
    p = subprocess.run([CLI, str(tmp_path / "c.r1cs"), str(tmp_path / "w.wtns")], capture_output=True, text=True)
    assert p.returncode == 2 and "3 elements" in p.stderr
    p = subprocess.run([CLI, str(tmp_path / "c.r1cs"), str(tmp_path / "c.r1cs")], capture_output=True, text=True)
    assert p.returncode == 2 and "bad magic" in p.stderr


# -- fixture extensions: list-form combinations, Montgomery helpers, planted systems -----------------------------------------
EDGE_COEFS = [0, 1, F.R - 1, 2, F.R - 2, (F.R + 1) // 2, F.MONT_R, F.MONT_R_INV, F.MONT_R2, (1 << 255) % F.R]


def _lc_bytes_dict_only(lc):
    """the writer's dict form as it was before list-form combinations existed (a frozen copy)"""
    out = [struct.pack("<I", len(lc))]
    for wire, c in sorted(lc.items()):
        out.append(struct.pack("<I", wire) + (c % F.R).to_bytes(32, "little"))
    return b"".join(out)


def test_dict_form_output_is_unchanged(pkg):
    rnd = random.Random(31)
    unreduced = [({3: -1, 1: F.R + 5}, {0: 2 * F.R - 1}, {4: -7, 2: 1 << 300})]
    rand = [tuple({rnd.randrange(50): rnd.choice([rnd.randrange(F.R), -rnd.randrange(F.R), 1, F.R - 1])
                   for _ in range(rnd.randrange(6))} for _ in range(3)) for _ in range(40)]
    for cons in (CONS, unreduced, rand, F.derive_r1cs(_poseidon_builder())):
        want = b"".join(_lc_bytes_dict_only(a) + _lc_bytes_dict_only(b) + _lc_bytes_dict_only(c) for a, b, c in cons)
        assert F.constraints_section(cons) == want


def test_list_form_round_trip(pkg):
    lists = [([(1, 1), (1, F.R - 1), (0, 5), (1, 3)], [], [(3, 0), (3, 0)]),
             ([(4, c) for c in EDGE_COEFS], [(0, c) for c in reversed(EDGE_COEFS)], [(2, 1), (4, F.R - 1), (2, 7)]),
             ([], [(4, 1)] * 5, [])]
    r = _load(F.write_r1cs(5, lists))
    assert r.info["n_constraints"] == 3
    assert (r.info["n_factors_a"], r.info["n_factors_b"], r.info["n_factors_c"]) == (4 + len(EDGE_COEFS), len(EDGE_COEFS) + 5, 5)
    # list form writes pairs as given: order and duplicates in the bytes, and the loader refuses r and 2^256 - 1
    sec = F.constraints_section(lists[:1])
    assert struct.unpack_from("<I", sec, 0)[0] == 4 and struct.unpack_from("<I", sec, 4 + 36 * 3)[0] == 1
    for bad in (F.R, (1 << 256) - 1):
        _rejects(F.write_r1cs(5, [([(1, 1), (2, bad)], [], [])]), "constraint 0 has a coefficient >= r")
    _rejects(F.write_r1cs(5, [([(1, 1)], [], [(5, 1)])]), "references wire 5")


def test_list_checker_agrees_with_dict_checker(pkg):
    rnd = random.Random(32)
    for _ in range(30):
        dicts = [tuple({rnd.randrange(8): rnd.choice([1, F.R - 1, rnd.randrange(F.R)]) for _ in range(rnd.randrange(5))}
                       for _ in range(3)) for _ in range(12)]
        lists = [tuple(list(lc.items())[::-1] for lc in con) for con in dicts]
        w = [1] + [rnd.randrange(F.R) for _ in range(7)]
        assert F.check(lists, w) == F.check(dicts, w)
        # satisfy constraint 0 by construction of C, then compare again
        a, b, c = dicts[0]
        dicts[0] = (a, b, {0: F._dot(a, w) * F._dot(b, w) % F.R})
        lists[0] = (list(a.items()), list(b.items()), [(0, 1), (0, F._dot(a, w) * F._dot(b, w) - 1)])
        assert F.check_constraint(dicts[0], w) and F.check_constraint(lists[0], w)
        assert F.check(lists, w) == F.check(dicts, w)
    # duplicates are summed
    w = [1, 10, 20]
    assert F.check_constraint(([(1, 2), (1, 3)], [(0, 1)], [(1, 5)]), w)
    assert F.check_constraint(([(2, 1), (2, F.R - 1)], [(1, 1)], []), w)
    assert not F.check_constraint(([(1, 2), (1, 3)], [(0, 1)], [(1, 4)]), w)


def test_montgomery_helpers(pkg):
    rnd = random.Random(33)
    for x in [0, 1, 2, F.R - 1] + [rnd.randrange(F.R) for _ in range(100)]:
        assert F.from_montgomery(F.to_montgomery(x)) == x and F.to_montgomery(F.from_montgomery(x)) == x
        assert F.to_montgomery(x) == x * (1 << 256) % F.R
    assert F.to_montgomery(1) == F.MONT_R and F.MONT_R * F.MONT_R_INV % F.R == 1 and F.MONT_R2 == F.MONT_R ** 2 % F.R


def test_planted_systems_are_satisfied(pkg):
    rnd = random.Random(34)
    for pool, dup, edge in (([1, F.R - 1, None], False, False), (EDGE_COEFS + [None], True, True), ([None], True, False)):
        shapes = [dict(a=rnd.randrange(6), b=rnd.randrange(6), c=rnd.randrange(6), dup=dup, edge=edge) for _ in range(60)]
        shapes += [dict(a=4, b=2, c=0, out=False), dict(a=0, b=3, c=0, out=False), dict(a=0, b=0, c=0, out=False)]
        P = F.planted_system(rnd, 8, shapes, pool)
        assert P.n_wires == 1 + 60 + 1 + 8 and P.free[-1] == P.n_wires - 1
        if edge:
            assert all(any(w == 0 for w, _ in lc) and any(w == P.n_wires - 1 for w, _ in lc)
                       for a, b, c in P.constraints[:60] for lc, n in ((a, 2), (b, 2)) if len(lc) >= n)
        if dup:
            assert any(len({w for w, _ in lc}) < len(lc) for con in P.constraints for lc in con)
        for j, (a, b, c) in enumerate(P.constraints[60:]):
            assert not c and all(w == P.zero_wire for w, _ in a)
        for _ in range(4):
            w = P.complete(rnd)
            assert w[0] == 1 and w[P.zero_wire] == 0 and all(0 <= x < F.R for x in w)
            assert F.check(P.constraints, w) == (0xFFFFFFFF, 0)
        # an output wire changed: its own constraint (C holds it with a nonzero coefficient) is the first to fail
        w[5] = (w[5] + 1) % F.R
        first, n = F.check(P.constraints, w)
        assert first == 4 and n >= 1
        # fixed free values are honoured
        w = P.complete(rnd, fixed={P.free[0]: 12345})
        assert w[P.free[0]] == 12345 and F.check(P.constraints, w) == (0xFFFFFFFF, 0)
