"""A powers-of-tau ceremony on an MI355X (r1cs/ceremony.hip, include/graph_witness_groth16_ceremony.h) on files of power 3 and 4.
The oracle of a contribution is the Python writer: a file written from the logs (tau, alpha, beta) holds after a contribution
with (tau', alpha', beta') exactly the bytes of the file written from the products, in whole and in pieces of five points.  The
record is recomputed by tests/ceremony_fixtures.py; the verification accepts the honest chain and names the rule that each
tampered file breaks."""
import ctypes
import functools
import math
import os
import random
import struct
import subprocess

import pytest

import cwc_import
from tests import ceremony_fixtures as CE
from tests import contribution_fixtures as CF
from tests import g2_subgroup_fixtures as SF
from tests import groth16_fixtures as GF
from tests import ptau_fixtures as PF
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
R = GF.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "circom-witnesscalc_amd")
SEED = bytes(range(9, 41))
_rnd = random.Random(950)
TAU, ALPHA, BETA = (_rnd.randrange(2, R) for _ in range(3))
FIRST, SECOND = (tuple(_rnd.randrange(2, R) for _ in range(3)) for _ in range(2))

pytestmark = pytest.mark.gpu


def split(image):
    """[(id, body)] of a binfile in file order"""
    (n,), off, out = struct.unpack_from("<I", image, 8), 12, []
    for _ in range(n):
        sid, size = struct.unpack_from("<IQ", image, off)
        out.append((sid, image[off + 12:off + 12 + size]))
        off += 12 + size
    assert off == len(image)
    return out


def join(sections):
    return b"ptau" + struct.pack("<II", 1, len(sections)) + b"".join(GF.section(i, b) for i, b in sections)


def with_section(image, sid, body):
    return join([(i, body if i == sid else b) for i, b in split(image)])


def products(*triples):
    return tuple(math.prod(t[j] for t in triples) % R for j in range(3))


@functools.lru_cache(maxsize=None)
def chain(power):
    """ptau_new and two contributions: [(file, digest)]"""
    f0 = PKG.ptau_new(power)
    f1, d1 = PKG.ptau_contribute(f0, name="first", secrets=FIRST)
    f2, d2 = PKG.ptau_contribute(f1, name="second", secrets=SECOND)
    return (f0, None), (f1, d1), (f2, d2)


def verdict(call, *args):
    """(rc, message) of gwb_ptau_verify or gwb_ptau_verify_step through the C ABI"""
    st = PKG.GwStatus()
    rc = call(*args, ctypes.byref(st))
    msg = ctypes.string_at(st.error_msg).decode() if st.error_msg else ""
    return rc, msg


def verify_rc(image, flags=0):
    n = ctypes.c_size_t(0)
    return verdict(PKG.r1cs_lib().gwb_ptau_verify, image, len(image), flags, SEED, None, ctypes.byref(n))


def step_rc(prev, nxt):
    return verdict(PKG.r1cs_lib().gwb_ptau_verify_step, prev, len(prev), nxt, len(nxt), SEED)


# -- 1. the contribution's bytes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", [3, 4])
def test_a_contribution_gives_the_file_of_the_products(power):
    out, digest = PKG.ptau_contribute(PF.write_ptau(power, TAU, ALPHA, BETA), secrets=FIRST)
    want = PF.sections(power, *products((TAU, ALPHA, BETA), FIRST))
    got = split(out)
    assert [i for i, _ in got] == [1, 2, 3, 4, 5, 6, 7]
    for sid, body in got[:6]:
        assert body == want[sid], sid
    assert PKG.ptau_info(out) == {"power": power, "ceremony_power": power, "prepared": False, "n_contributions": 1}
    assert PKG.ptau_contributions(out)[0]["next_challenge"] == digest


def test_two_contributions_from_a_new_file():
    (f0, _), (f1, _), (f2, _) = chain(3)
    for image, logs in ((f1, FIRST), (f2, products(FIRST, SECOND))):
        want = PF.sections(3, *logs)
        assert dict(split(image)[:6]) == {sid: want[sid] for sid in range(1, 7)}


@pytest.mark.parametrize("power", [3, 4])
def test_a_contribution_in_pieces_of_five_points(power, monkeypatch):
    """pieces end inside every section (31 and 16 points at power 4: the last piece is short), so a wrong first index of a piece
    shows in every point after the first seam"""
    monkeypatch.setenv("CWC_CONTRIBUTE_CHUNK", "5")
    out, _ = PKG.ptau_contribute(PF.write_ptau(power, TAU, ALPHA, BETA), secrets=SECOND)
    want = PF.sections(power, *products((TAU, ALPHA, BETA), SECOND))
    assert dict(split(out)[:6]) == {sid: want[sid] for sid in range(1, 7)}


# -- 2. the record --------------------------------------------------------------------------------------------------------------------
def test_the_record_of_a_contribution():
    (f0, _), (f1, d1), (f2, d2) = chain(3)
    challenge = CE.first_challenge(dict(split(f0))[1])
    for k, (image, digest, secrets, logs) in enumerate(((f1, d1, FIRST, FIRST), (f2, d2, SECOND, products(FIRST, SECOND)))):
        recs = CE.read_section7(dict(split(image))[7])
        assert len(recs) == k + 1
        rec = recs[k]
        assert rec.pts["tau_g1"] is not None and {n: rec.pts[n] for n in ("tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2")} == CE.anchors(*logs)
        secs = dict(split(image))
        assert (secs[2][64:128], secs[3][128:256], secs[4][:64], secs[5][:64], secs[6]) == tuple(
            (GF.g2_bytes if n.endswith("g2") else GF.g1_bytes)(rec.pts[n]) for n in ("tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2"))
        for j, nm in enumerate(CE.SECRETS):
            g1_s, g1_sx = rec.pts[nm + "_g1_s"], rec.pts[nm + "_g1_sx"]
            assert g1_s is not None and GF.G1.to_affine(GF.G1.mul(g1_s, secrets[j])) == g1_sx
            g2_sp = CE.key_point(challenge, j, g1_s, g1_sx)
            assert GF.G2.to_affine(GF.G2.mul(g2_sp, secrets[j])) == rec.pts[nm + "_g2_spx"]
        assert rec.next_challenge == CF.H(challenge + rec.pub()) == digest
        assert rec.partial_hash == bytes(216) and rec.type == 0 and rec.params == CF.name_params(("first", "second")[k])
        got = PKG.ptau_contributions(image)[k]
        assert got["name"] == ("first", "second")[k] and all(got[n] == b for n, b in rec.canonical().items())
        challenge = rec.next_challenge
    assert [r.stored() for r in CE.read_section7(dict(split(f2))[7])[:1]] == [r.stored() for r in CE.read_section7(dict(split(f1))[7])]
    nonces = {PKG.ptau_contributions(f2)[k][n + "_g1_s"] for k in range(2) for n in CE.SECRETS}
    assert len(nonces) == 6  # a nonce of its own per key


def test_prepared_sections_are_dropped_and_unknown_ones_carried():
    secs = PF.sections(3, TAU, ALPHA, BETA, prepared=True)
    secs[99] = b"an unknown section"
    image = PF.assemble(secs, order=[1, 99, 12, 2, 3, 13, 4, 5, 6, 14, 15, 7])
    assert PKG.ptau_info(image)["prepared"]
    out, _ = PKG.ptau_contribute(image, secrets=FIRST)
    got = split(out)
    assert [i for i, _ in got] == [1, 99, 2, 3, 4, 5, 6, 7] and dict(got)[99] == secs[99] and dict(got)[1] == secs[1]
    want = PF.sections(3, *products((TAU, ALPHA, BETA), FIRST))
    assert all(dict(got)[sid] == want[sid] for sid in range(2, 7))
    assert not PKG.ptau_info(out)["prepared"]
    del secs[7]  # a file without section 7 gets one at the end
    out, _ = PKG.ptau_contribute(PF.assemble({i: secs[i] for i in range(1, 7)}), secrets=FIRST)
    assert [i for i, _ in split(out)] == [1, 2, 3, 4, 5, 6, 7] and len(PKG.ptau_contributions(out)) == 1


def test_a_point_fault_is_named_as_the_setup_names_it():
    secs = PF.sections(3, TAU, ALPHA, BETA)
    secs[2] = secs[2][:64 * 9 + 32] + GF.lem(1) + secs[2][64 * 10:]
    with pytest.raises(PKG.WitnessCalcError, match=r"^ptau: section 2 \(tauG1\) point 9 is not on the G1 curve$"):
        PKG.ptau_contribute(PF.assemble(secs), secrets=FIRST)
    secs = PF.sections(3, TAU, ALPHA, BETA)
    secs[3] = secs[3][:128 * 5] + GF.Q.to_bytes(32, "little") + secs[3][128 * 5 + 32:]
    with pytest.raises(PKG.WitnessCalcError, match=r"^ptau: section 3 \(tauG2\) point 5 has a coordinate >= q$"):
        PKG.ptau_contribute(PF.assemble(secs), secrets=FIRST)


# -- 3. the verification ------------------------------------------------------------------------------------------------------------
def test_the_honest_chain_is_accepted():
    (f0, _), (f1, d1), (f2, d2) = chain(3)
    assert PKG.ptau_verify(f0, seed=SEED) == [] and PKG.ptau_verify(f1, seed=SEED) == [d1]
    assert PKG.ptau_verify(f2, seed=SEED) == [d1, d2] and PKG.ptau_verify(f2) == [d1, d2] and PKG.ptau_verify(f2, records=False, seed=SEED) == [d1, d2]
    PKG.ptau_verify_step(f0, f1, seed=SEED)
    PKG.ptau_verify_step(f1, f2)
    assert PKG.ptau_verify(chain(4)[2][0], seed=SEED) == [chain(4)[1][1], chain(4)[2][1]]
    rc, msg = step_rc(f0, f2)
    assert rc == 1 and msg == "ptau step: section 7 of the next file has 2 contributions, the previous file 0: exactly one more is expected"
    rc, msg = step_rc(f1, f1)
    assert rc == 1 and "exactly one more is expected" in msg
    rc, msg = step_rc(chain(4)[0][0], f1)
    assert rc == 1 and msg == "ptau step: section 1 (header) differs from the previous file's"


def rewritten(image, k, change, rechain=True):
    """`image` with record k (0-based) changed by change(record); rechain: its nextChallenge is made again from the challenge
    before it, as a forger would"""
    secs = dict(split(image))
    recs = CE.read_section7(secs[7])
    change(recs[k])
    if rechain:
        before = recs[k - 1].next_challenge if k else CE.first_challenge(secs[1])
        recs[k].next_challenge = CF.H(before + recs[k].pub())
    return with_section(image, 7, CE.write_section7(recs))


def test_tampered_records_are_refused():
    (f0, _), (f1, _), (f2, _) = chain(3)
    other = GF.G2.to_affine(GF.G2.gen_mul_jac(5))

    def swap(rec):
        rec.pts["alpha_g2_spx"] = other

    rc, msg = verify_rc(rewritten(f2, 0, swap, rechain=False))
    assert rc == 1 and msg == "ptau: contribution 1: nextChallenge is not that of the challenge before the record and the record's points"
    rc, msg = verify_rc(rewritten(f2, 1, swap))
    assert rc == 1 and msg == "ptau: contribution 2: alpha_g1_sx is not alpha_g1_s times the secret that alpha_g2_spx proves"
    rc, msg = step_rc(f1, rewritten(f2, 1, swap))
    assert rc == 1 and msg == "ptau: contribution 2: alpha_g1_sx is not alpha_g1_s times the secret that alpha_g2_spx proves"

    def infinity(rec):
        rec.pts["beta_g1_s"] = None

    rc, msg = verify_rc(rewritten(f2, 1, infinity))
    assert rc == 1 and msg == "ptau: contribution 2: beta_g1_s is the point at infinity"
    torsion = SF.exact_order(random.Random(5), SF.SMALL[0])

    def off_subgroup(rec):
        rec.pts["tau_g2_spx"] = GF.G2.to_affine(GF.G2.add(GF.G2.jac(rec.pts["tau_g2_spx"]), GF.G2.jac(torsion)))

    rc, msg = verify_rc(rewritten(f2, 1, off_subgroup))
    assert rc == 1 and msg == "ptau: contribution 2: tau_g2_spx is not in the order-r subgroup of G2"

    # a record whose after-values are not the file's: the first file's record over the second file's points
    rc, msg = verify_rc(with_section(f2, 7, dict(split(f1))[7]))
    assert rc == 1 and msg == "ptau: tauG1[1] of the file is not the after-value of the last contribution"
    # a previous alphaG1 that the proven secret does not lead to the record's: the second record alone over the generators
    recs = CE.read_section7(dict(split(f2))[7])
    recs[1].next_challenge = CF.H(CE.first_challenge(dict(split(f2))[1]) + recs[1].pub())
    rc, msg = verify_rc(with_section(f2, 7, CE.write_section7(recs[1:])))
    assert rc == 1 and msg == "ptau: contribution 1: tau_g1_sx is not tau_g1_s times the secret that tau_g2_spx proves"  # its challenge point is another
    rc, msg = verify_rc(with_section(f0, 7, dict(split(f1))[7]))
    assert rc == 1 and msg == "ptau: tauG1[1] of the file is not the after-value of the last contribution"
    rc, msg = verify_rc(with_section(f1, 7, CE.NO_RECORDS))
    assert rc == 1 and msg == "ptau: tauG1[1] of the file is not the generator, and no contribution accounts for it"

    # an earlier record altered, for the step check
    def rename(rec):
        rec.partial_hash = bytes([1]) + rec.partial_hash[1:]

    rc, msg = step_rc(f1, rewritten(f2, 0, rename, rechain=False))
    assert rc == 1 and msg == "ptau step: section 7: contribution 1 is not the previous file's"


def test_a_record_under_another_challenge_derivation():
    """the fixture's record with a challenge point derived otherwise: the proofs of knowledge fail, the points alone pass"""
    def derive(challenge, j, g1_s, g1_sx):
        return CF.hash_to_g2(CF.H(b"another derivation" + CE.key_transcript(challenge, j, g1_s, g1_sx)))

    secs = PF.sections(3, *products((TAU, ALPHA, BETA), FIRST))
    rec = CE.contribution(CE.first_challenge(secs[1]), (1, 1, 1), products((TAU, ALPHA, BETA), FIRST), (3, 5, 7), derive=derive)
    secs[7] = CE.write_section7([rec])
    image = PF.assemble(secs)
    rc, msg = verify_rc(image)
    assert rc == 1 and msg == "ptau: contribution 1: tau_g1_sx is not tau_g1_s times the secret that tau_g2_spx proves"
    assert PKG.ptau_verify(image, records=False, seed=SEED) == [rec.next_challenge]
    honest = CE.contribution(CE.first_challenge(secs[1]), (1, 1, 1), products((TAU, ALPHA, BETA), FIRST), (3, 5, 7))
    secs[7] = CE.write_section7([honest])
    assert PKG.ptau_verify(PF.assemble(secs), seed=SEED) == [honest.next_challenge]  # the fixture's own record is accepted


@pytest.mark.parametrize("power", [3, 4])
def test_the_whole_file_check_reads_every_point(power):
    f1 = chain(power)[1][0]
    secs, n = dict(split(f1)), 1 << power
    foreign = GF.g1_bytes(GF.G1.to_affine(GF.G1.gen_mul_jac(12345)))
    last = with_section(f1, 2, secs[2][:-64] + foreign)
    rc, msg = verify_rc(last)
    assert rc == 1 and msg == "ptau: section 2 (tauG1): the points are not consecutive powers of the tau of section 3"
    PKG.ptau_check_powers(last, power - 1, seed=SEED)  # the prefix check does not read the last point
    assert step_rc(chain(power)[0][0], last) == (1, msg)
    rc, msg = verify_rc(with_section(f1, 4, secs[4][:-64] + foreign), flags=PKG.PTAU_VERIFY_SKIP_RECORDS)
    assert rc == 1 and msg == "ptau: section 4 (alphaTauG1): the points are not alphaTauG1[0] times the powers of tau"
    rc, msg = verify_rc(with_section(f1, 5, secs[5][:64 * (n - 2)] + foreign + secs[5][64 * (n - 1):]))
    assert rc == 1 and msg == "ptau: section 5 (betaTauG1): the points are not betaTauG1[0] times the powers of tau"
    rc, msg = verify_rc(with_section(f1, 3, secs[3][:-128] + GF.g2_bytes(GF.G2.to_affine(GF.G2.gen_mul_jac(12345)))))
    assert rc == 1 and msg == "ptau: section 3 (tauG2): the points are not the powers of the tau of section 2"
    torsion = SF.exact_order(random.Random(6), SF.SMALL[0])
    mixed = GF.G2.to_affine(GF.G2.add(GF.G2.gen_mul_jac(pow(FIRST[0], n - 1, R)), GF.G2.jac(torsion)))
    rc, msg = verify_rc(with_section(f1, 3, secs[3][:-128] + GF.g2_bytes(mixed)))
    assert rc == 1 and msg == "ptau: section 3 (tauG2) point %d is not in the order-r subgroup of G2" % (n - 1)
    rc, msg = verify_rc(with_section(f1, 6, GF.g2_bytes(GF.G2.to_affine(GF.G2.gen_mul_jac(7)))))
    assert rc == 1 and msg == "ptau: betaG2 of the file is not the after-value of the last contribution"


# -- 4. end to end ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def smallest_system():
    """the planted system of test_gpu_groth16_setup.py::power_case for the domain 2^2 (construction restated): `.r1cs` bytes, R1cs"""
    p = 2
    n_c = (1 << p) - 1 - random.Random(p).randrange(0, 1 << (p - 1))
    rnd = random.Random(100 + p)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(n_c)]
    pl = F.planted_system(rnd, 6, shapes, [1, R - 1, 2, F.MONT_R, None])
    data = F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=0, n_pub_in=0)
    r1 = PKG.R1cs(data)
    assert r1.qap_info()["domain_power"] == p
    return data, r1


def test_a_ceremony_feeds_the_key_setup():
    """ptau_new -> two contributions -> prepare phase 2 -> the key with delta = 1 -> the key check with the powers check"""
    _, r1 = smallest_system()
    f2 = chain(3)[2][0]
    prepared = PKG.ptau_prepare_phase2(f2)
    assert PKG.ptau_info(prepared) == {"power": 3, "ceremony_power": 3, "prepared": True, "n_contributions": 2}
    key = PKG.groth16_setup_ptau(r1, prepared, delta=1)
    assert PKG.groth16_verify_key(key, r1, prepared, check_ptau=True, seed=SEED) == []
    assert PKG.ptau_verify(prepared, seed=SEED) == [chain(3)[1][1], chain(3)[2][1]]


def test_cli_chain(tmp_path):
    path = lambda name: str(tmp_path / name)  # noqa: E731
    cli = os.path.join(BIN, "powersoftau")
    run = lambda *args: subprocess.run([cli] + list(args), capture_output=True, text=True, timeout=300)  # noqa: E731
    (f0, _), (f1, d1), (f2, d2) = chain(3)
    p = run("new", "3", path("f0.ptau"))
    assert p.returncode == 0 and (tmp_path / "f0.ptau").read_bytes() == f0, p
    hashes = []
    for k, secrets in enumerate((FIRST, SECOND)):
        (tmp_path / "s.txt").write_text(" ".join(str(x) for x in secrets) + "\n")
        p = run("contribute", "--name", ("first", "second")[k], "--secrets", path("s.txt"), path("f%d.ptau" % k), path("f%d.ptau" % (k + 1)))
        assert p.returncode == 0 and p.stderr == "", p
        hashes.append(p.stdout.strip())
    # the records differ from the chain's by their nonces alone: sections 1 to 6 are the same bytes
    assert split((tmp_path / "f2.ptau").read_bytes())[:6] == split(f2)[:6]
    assert [r["next_challenge"].hex() for r in PKG.ptau_contributions((tmp_path / "f2.ptau").read_bytes())] == hashes and d1.hex() not in hashes
    p = run("contribute", path("f2.ptau"), path("f3.ptau"))  # drawn secrets
    assert p.returncode == 0 and len(p.stdout.strip()) == 128, p
    hashes.append(p.stdout.strip())
    p = run("verify", path("f3.ptau"))
    assert p.returncode == 0 and p.stdout.splitlines() == ["OK! power 3, 3 contributions"] + hashes, p
    p = run("verify", "--skip-records", path("f3.ptau"))
    assert p.returncode == 0 and p.stdout.splitlines()[0] == "OK! power 3, 3 contributions (not verified)", p
    p = run("verify-step", path("f2.ptau"), path("f3.ptau"))
    assert p.returncode == 0 and p.stdout.startswith("OK! ") and p.stdout.splitlines()[1:] == hashes[2:], p
    p = run("verify-step", path("f0.ptau"), path("f2.ptau"))
    assert p.returncode == 1 and p.stderr.startswith("INVALID: ptau step: section 7 of the next file has 2 contributions") and p.stdout == "", p
    (tmp_path / "bad.ptau").write_bytes(with_section(f2, 2, dict(split(f2))[2][:-64] + dict(split(f2))[2][64:128]))
    p = run("verify", path("bad.ptau"))
    assert p.returncode == 1 and p.stderr == "INVALID: ptau: section 2 (tauG1): the points are not consecutive powers of the tau of section 3\n", p
    (tmp_path / "junk.ptau").write_bytes(f2[:-1])
    p = run("verify", path("junk.ptau"))
    assert p.returncode == 2 and p.stderr.startswith("error: ptau: "), p


def test_phase_timer():
    PKG.ptau_contribute(chain(4)[0][0], secrets=FIRST)
    ms = PKG.ptau_contribute_phase_ms()
    assert list(ms) == ["load", "scalars", "mul_g1", "mul_g2", "affine"] == list(PKG.PTAU_CONTRIBUTE_PHASES)
    assert all(math.isfinite(x) and x > 0 for x in ms.values()), ms
