"""Section 4 of a zkey on the host, without a GPU: a Groth16 handle without an R1cs, gwb_zkey_check_r1cs against section 4 written
from plain integers (tests/zkey_coefs_fixtures.py: c R^2 mod r, R = 2^256) in equivalent and in differing forms, what the lazy build
refuses at its first use (and the loader must not), deterministic mutants of the section, and the four-argument CLI's errors."""
import os
import random
import struct
import subprocess

import pytest

import cwc_import
from tests import groth16_fixtures as GF
from tests import r1cs_fixtures as F
from tests import zkey_coefs_fixtures as ZF

PKG = cwc_import.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = F.R
N_PUB_OUT, N_PUB_IN = 1, 2
N_PUB = N_PUB_OUT + N_PUB_IN


@pytest.fixture(scope="module")
def system():
    """planted system, its Trapdoor zkey, the entries of its section 4 and its R1cs"""
    rnd = random.Random(31)
    shapes = [{"a": rnd.randrange(1, 4), "b": rnd.randrange(1, 4), "c": rnd.randrange(0, 3)} for _ in range(6)]
    pl = F.planted_system(rnd, 5, shapes, [1, R - 1, 2, F.MONT_R, None])
    T = GF.Trapdoor(pl.constraints, pl.n_wires, N_PUB, seed=5)
    ent = ZF.entries_of(pl.constraints, N_PUB)
    return pl, T, ent, _r1cs(pl)


def _r1cs(pl, n_wires=None, n_pub_in=N_PUB_IN, constraints=None):
    return PKG.R1cs(F.write_r1cs(n_wires or pl.n_wires, constraints or pl.constraints, n_pub_out=N_PUB_OUT, n_pub_in=n_pub_in))


def _key(T, entries):
    return PKG.Groth16(ZF.zkey_of(T, entries))


def test_constructs_without_an_r1cs(system):
    pl, T, ent, r1 = system
    g = PKG.Groth16(ZF.zkey_of(T))
    assert g.r1cs is None
    assert g.info == {"n_vars": pl.n_wires, "n_public": N_PUB, "domain_size": T.n, "n_coefs": len(ent)}
    assert g.qap_info() == {"n_rows": len(pl.constraints) + N_PUB + 1, "domain_power": T.n.bit_length() - 1, "domain_size": T.n,
                            "workspace_bytes_per_row": 64 * T.n}
    with pytest.raises(PKG.WitnessCalcError, match="no R1cs"):
        g.check_r1cs()
    for t in (0, 1, 2, 4, 8, 16, 32, 64):
        g.set_tile_width(t)
    for t in (3, 65, 128):
        with pytest.raises(PKG.WitnessCalcError):
            g.set_tile_width(t)


def test_check_r1cs_accepts_equivalent_sections(system):
    pl, T, ent, r1 = system
    _key(T, ent).check_r1cs(r1)
    PKG.Groth16(ZF.zkey_of(T), r1).check_r1cs()  # the handle's own R1cs by default
    rnd = random.Random(32)
    shuffled = list(ent)
    rnd.shuffle(shuffled)
    _key(T, shuffled).check_r1cs(r1)
    m, c, s, v = ent[3]
    part = rnd.randrange(R)
    split = ent[:3] + [(m, c, s, part)] + ent[4:] + [(m, c, s, (v - part) % R)]
    _key(T, split).check_r1cs(r1)
    x = rnd.randrange(1, R)
    cancel = ent + [(1, 2, pl.n_wires - 1, x), (1, 2, pl.n_wires - 1, R - x)]
    _key(T, cancel).check_r1cs(r1)
    zeros = [(0, T.n - 1, 0, 0)] + ent + [(1, 0, 1, 0), (0, 3, pl.n_wires - 1, 0)]
    _key(T, zeros).check_r1cs(r1)
    everything = list(split) + cancel[len(ent):] + [(1, 0, 1, 0)]
    rnd.shuffle(everything)
    _key(T, everything).check_r1cs(r1)


def _differs(T, entries, r1, reference):
    key = ZF.first_difference(entries, reference)
    assert key is not None
    with pytest.raises(PKG.WitnessCalcError) as e:
        _key(T, entries).check_r1cs(r1)
    assert str(e.value) == ZF.difference_message(key)
    return key


def test_check_r1cs_names_the_smallest_difference(system):
    pl, T, ent, r1 = system
    n_c = len(pl.constraints)
    # one changed value
    k = next(i for i, e in enumerate(ent) if e[1] == 2)
    m, c, s, v = ent[k]
    assert _differs(T, ent[:k] + [(m, c, s, (v + 1) % R)] + ent[k + 1:], r1, ent)[0] == 2
    # a term moved to another signal, and to the other matrix
    k = next(i for i, e in enumerate(ent) if e[1] == 4 and e[0] == 1)
    m, c, s, v = ent[k]
    other = next(w for w in range(pl.n_wires) if all(e[:3] != (m, c, w) for e in ent))
    _differs(T, ent[:k] + [(m, c, other, v)] + ent[k + 1:], r1, ent)
    _differs(T, ent[:k] + [(1 - m, c, s, v)] + ent[k + 1:], r1, ent)
    # a missing public row, an extra term
    k = next(i for i, e in enumerate(ent) if e[1] == n_c + 2)
    assert _differs(T, ent[:k] + ent[k + 1:], r1, ent) == (n_c + 2, 0, 2)
    assert _differs(T, ent + [(1, n_c + 1, 0, 7)], r1, ent) == (n_c + 1, 1, 0)
    assert _differs(T, ent + [(0, T.n - 1, pl.n_wires - 1, R - 1)], r1, ent) == (T.n - 1, 0, pl.n_wires - 1)
    # several differences: the smallest is named
    many = [e for e in ent if e[1] != 1] + [(0, 5, 0, 3)]
    assert _differs(T, many, r1, ent)[0] == 1


def test_check_r1cs_on_pairs_that_differ_only_in_size_fields(system):
    """one public input fewer in the .r1cs: its last public row is missing, and that row is named; one unused wire more: the
    terms are the same, and the size field is named"""
    pl, T, ent, r1 = system
    n_c = len(pl.constraints)
    g = _key(T, ent)
    with pytest.raises(PKG.WitnessCalcError) as e:
        g.check_r1cs(_r1cs(pl, n_pub_in=N_PUB_IN - 1))
    assert str(e.value) == ZF.difference_message((n_c + N_PUB, 0, N_PUB))
    with pytest.raises(PKG.WitnessCalcError, match=r"^zkey: .*nVars %d != r1cs nWires %d" % (pl.n_wires, pl.n_wires + 1)):
        g.check_r1cs(_r1cs(pl, n_wires=pl.n_wires + 1))


def _first_use(zkey):
    g = PKG.Groth16(zkey)  # the loader accepts it
    with pytest.raises(PKG.WitnessCalcError) as e:
        g.qap_info()
    assert str(e.value).startswith("zkey:")
    return g, str(e.value)


def test_first_use_refusals(system):
    pl, T, ent, r1 = system
    k = len(ent) // 2
    m, c, s, _ = ent[k]
    for raw in (R, (1 << 256) - 1):
        bad = ent[:k] + [(m, c, s, raw.to_bytes(32, "little"))] + ent[k + 1:]
        g, msg = _first_use(ZF.zkey_of(T, bad))
        assert "coefficient %d " % k in msg and ">= r" in msg and "constraint %d" % c in msg and "signal %d" % s in msg
        with pytest.raises(PKG.WitnessCalcError, match="^zkey: coefficient %d .*>= r" % k):
            g.check_r1cs(r1)
        # refused again at the next use: nothing half-built is kept
        with pytest.raises(PKG.WitnessCalcError, match="^zkey: coefficient %d " % k):
            g.qap_info()
    g, msg = _first_use(T.zkey)  # an empty section 4
    assert g.info["n_coefs"] == 0 and "no coefficients" in msg and ".r1cs" in msg
    with pytest.raises(PKG.WitnessCalcError, match="^zkey: section 4 differs from the r1cs at constraint 0, matrix A"):
        g.check_r1cs(r1)


def test_first_use_refuses_domain_size_1():
    """a one-point domain: nVars = 1, nPublic = 0, one H point, the row of wire 0 in section 4"""
    g1 = GF.G1.gen_muls([2, 3, 5, 7])
    g2 = GF.G2.gen_muls([3, 11, 5])
    z = GF.write_zkey(1, 0, 1, g1[0], g1[1], g2[0], g2[1], g1[2], g2[2], [g1[3]], [g1[3]], [g1[3]], [g2[0]], [], [g1[3]])
    _, msg = _first_use(ZF.splice(z, ZF.section4([(0, 0, 0, 1)])))
    assert "domainSize 1" in msg


def _outcome(zkey, r1):
    """'load' (refused by the loader), 'use' (refused at first use) or 'ok'; every message starts with zkey:"""
    try:
        g = PKG.Groth16(zkey)
    except PKG.WitnessCalcError as e:
        assert str(e).startswith("zkey:"), e
        return "load"
    out = "ok"
    try:
        g.qap_info()
    except PKG.WitnessCalcError as e:
        assert str(e).startswith("zkey:"), e
        out = "use"
    try:
        g.check_r1cs(r1)
    except PKG.WitnessCalcError as e:
        assert str(e).startswith("zkey:"), e
    return out


def test_deterministic_mutants_never_crash(system):
    pl, T, ent, r1 = system
    body = ZF.section4(ent)
    n = len(ent)
    assert _outcome(ZF.splice(T.zkey, body), r1) == "ok"
    # every field of the first, a middle and the last entry at its bound and one past it
    bounds = ((0, 1), (4, T.n - 1), (8, pl.n_wires - 1))
    for k in (0, n // 2, n - 1):
        at = 4 + 44 * k
        for off, bound in bounds:
            for v, want in ((bound, ("ok",)), (bound + 1, ("load",)), (0xffffffff, ("load",))):
                m = body[:at + off] + struct.pack("<I", v) + body[at + off + 4:]
                assert _outcome(ZF.splice(T.zkey, m), r1) in want, (k, off, v)
        for v, want in ((R - 1, "ok"), (R, "use"), ((1 << 256) - 1, "use"), (0, "ok"), (1, "ok")):
            m = body[:at + 12] + v.to_bytes(32, "little") + body[at + 44:]
            assert _outcome(ZF.splice(T.zkey, m), r1) == want, (k, v)  # (value bytes alone never change what load does)
        # single value bytes
        for byte in (0, 15, 31):
            m = bytearray(body)
            m[at + 12 + byte] ^= 0x01
            below = int.from_bytes(m[at + 12:at + 44], "little") < R
            assert _outcome(ZF.splice(T.zkey, bytes(m)), r1) == ("ok" if below else "use")
    # truncations at every entry boundary and one byte to either side (the section header follows the body's length)
    for k in range(n + 1):
        for d in (-1, 0, 1):
            cut = 4 + 44 * k + d
            if 0 <= cut < len(body):
                assert _outcome(ZF.splice(T.zkey, body[:cut]), r1) == "load", cut
    assert _outcome(ZF.splice(T.zkey, body + b"\0"), r1) == "load"
    # counts
    assert _outcome(ZF.splice(T.zkey, ZF.section4(ent, count=0)), r1) == "load"
    assert _outcome(ZF.splice(T.zkey, ZF.section4(ent, count=n - 1)), r1) == "load"
    assert _outcome(ZF.splice(T.zkey, ZF.section4(ent, count=n + 1)), r1) == "load"
    assert _outcome(ZF.splice(T.zkey, ZF.section4(ent[:-1], count=n - 1)), r1) == "ok"  # (a consistent file: it lacks a public row)
    assert _outcome(ZF.splice(T.zkey, ZF.section4([], count=0)), r1) == "use"
    assert _outcome(ZF.splice(T.zkey, ZF.section4([], count=0xffffffff)), r1) == "load"
    # the whole file cut inside section 4
    z = ZF.zkey_of(T)
    start = z.index(body)
    for cut in (start, start + 4, start + 4 + 44, start + len(body) - 1):
        assert _outcome(z[:cut], r1) == "load"


def test_cli_four_argument_errors(tmp_path, system):
    pl, T, ent, r1 = system
    cli = os.path.join(ROOT, "circom-witnesscalc_amd", "groth16-prove")
    p = subprocess.run([cli, "a", "b", "c"], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr
    p = subprocess.run([cli, str(tmp_path / "no.zkey"), "b", "c", "d"], capture_output=True, text=True)
    assert p.returncode == 2 and "cannot read" in p.stderr
    zk = tmp_path / "c.zkey"
    zk.write_bytes(b"zkey" + bytes(8))
    wt = tmp_path / "w.wtns"
    wt.write_bytes(b"")
    out = [str(tmp_path / "p.json"), str(tmp_path / "q.json")]
    p = subprocess.run([cli, str(zk), str(wt)] + out, capture_output=True, text=True)
    assert p.returncode == 2 and "zkey:" in p.stderr
    p = subprocess.run([cli, str(zk), str(tmp_path / "no.wtns")] + out, capture_output=True, text=True)
    assert p.returncode == 2 and "cannot read" in p.stderr
    # parsed before the device is touched: a bad .wtns image, a witness of another size, a key without coefficients, a value >= r
    zk.write_bytes(ZF.zkey_of(T))
    p = subprocess.run([cli, str(zk), str(wt)] + out, capture_output=True, text=True)
    assert p.returncode == 2 and "wtns:" in p.stderr
    wt.write_bytes(ZF.wtns_image([1] + [0] * pl.n_wires))
    p = subprocess.run([cli, str(zk), str(wt)] + out, capture_output=True, text=True)
    assert p.returncode == 2 and "nVars" in p.stderr
    wt.write_bytes(ZF.wtns_image([1] + [0] * (pl.n_wires - 1)))
    zk.write_bytes(T.zkey)
    p = subprocess.run([cli, str(zk), str(wt)] + out, capture_output=True, text=True)
    assert p.returncode == 2 and "zkey: section 4 carries no coefficients" in p.stderr
    zk.write_bytes(ZF.zkey_of(T, ent[:-1] + [ent[-1][:3] + (R.to_bytes(32, "little"),)]))
    p = subprocess.run([cli, str(zk), str(wt)] + out, capture_output=True, text=True)
    assert p.returncode == 2 and ">= r" in p.stderr
    assert not os.path.exists(out[0]) and not os.path.exists(out[1])
