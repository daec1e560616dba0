"""The key check on an MI355X (groth16_verify_key: is this `.zkey` the honest key of this `.r1cs` and this `.ptau`?), the powers
check of a `.ptau` (ptau_check_powers) and the G2 linear-combination kernel both rest on (r1cs/contribute.hip).  The kernel is
tested through its aid on multiples of the G2 generator from bn254_gen_mul_batch_device, so the expected point is one more
fixed-base multiplication.  Files of known (tau, alpha, beta) come from tests/ptau_fixtures.py with the device's points, keys
from groth16_setup_ptau and groth16_contribute, which have tests of their own; every refusal is a file or a key with one thing
changed, and the message names what."""
import functools
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import cwc_import
from tests import contribution_fixtures as CF
from tests import g2_subgroup_fixtures as SF
from tests import groth16_fixtures as GF
from tests import ptau_fixtures as PF
from tests import r1cs_fixtures as F

PKG = cwc_import.load()
R, Q = F.R, GF.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "circom-witnesscalc_amd")
_rnd = random.Random(500)
TAU, ALPHA, BETA, D_A, D_B, OTHER = (_rnd.randrange(2, R) for _ in range(6))
HDR_ALPHA1, HDR_GAMMA2, HDR_DELTA1 = 84, 84 + 64 + 64 + 128, 84 + 64 + 64 + 128 + 128
MONT_INV = pow(GF.MONT, -1, Q)
SEED = bytes(range(3, 35))
REMADE = "the key remade from the circuit and the powers-of-tau file"

pytestmark = pytest.mark.gpu


# -- files and points (the small helpers of test_gpu_groth16_contribute.py, restated) ---------------------------------------------
def sections(zkey):
    """`.zkey` bytes -> {id: body}"""
    n_sec = struct.unpack_from("<I", zkey, 8)[0]
    off, out = 12, {}
    for _ in range(n_sec):
        sid, size = struct.unpack_from("<IQ", zkey, off)
        out[sid] = zkey[off + 12:off + 12 + size]
        off += 12 + size
    assert off == len(zkey)
    return out


def with_sections(zkey, **changed):
    """the key with the bodies of sections s<id> replaced"""
    secs = sections(zkey)
    for k, body in changed.items():
        secs[int(k[1:])] = body
    return b"zkey" + struct.pack("<II", 1, len(secs)) + b"".join(GF.section(i, secs[i]) for i in sorted(secs))


def patched(body, at, new):
    return body[:at] + new + body[at + len(new):]


def device_canonical(group, scalars):
    """[k] -> uint8 [n, 64 group]: k G, canonical affine, zero bytes for infinity (existing code)"""
    import torch
    arr = np.frombuffer(b"".join((k % R).to_bytes(32, "little") for k in scalars), dtype=np.uint8).reshape(len(scalars), 32)
    out = PKG.bn254_gen_mul_batch_device(torch.from_numpy(arr.copy()).cuda(), group)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def device_points(group, scalars):
    """the stored form (Montgomery) of k G, as the files hold it"""
    raw = device_canonical(group, scalars).tobytes()
    return b"".join(GF.lem(int.from_bytes(raw[o:o + 32], "little")) for o in range(0, len(raw), 32))


def _fq(b):
    return int.from_bytes(b, "little") * MONT_INV % Q


def g1_of(b):
    return None if not any(b) else (_fq(b[:32]), _fq(b[32:64]))


def g2_of(b):
    return None if not any(b) else ((_fq(b[:32]), _fq(b[32:64])), (_fq(b[64:96]), _fq(b[96:128])))


def g1_sum(b, c, sign=1):
    """stored b + sign * stored c, stored, on the Python curve"""
    q = g1_of(c) if sign == 1 else GF.G1.neg_aff(g1_of(c))
    return GF.g1_bytes(GF.G1.to_affine(GF.G1.add(GF.G1.jac(g1_of(b)), GF.G1.jac(q))))


def doubled(body, width):
    """(offset, the double of the stored point there) for the first point of `body` that is not infinity"""
    at = next(o for o in range(0, len(body), width) if any(body[o:o + width]))
    if width == 64:
        return at, GF.g1_bytes(GF.G1.to_affine(GF.G1.mul(g1_of(body[at:at + 64]), 2)))
    return at, GF.g2_bytes(GF.G2.to_affine(GF.G2.mul(g2_of(body[at:at + 128]), 2)))


def scale_stored(body, k):
    """every stored G1 point of `body` times k, through the scale aid (existing code)"""
    import torch
    canon = np.frombuffer(b"".join(_fq(body[o:o + 32]).to_bytes(32, "little") for o in range(0, len(body), 32)), dtype=np.uint8).reshape(-1, 64)
    got = PKG.bn254_g1_scale_batch_device(torch.from_numpy(canon.copy()).cuda(), k)
    torch.cuda.synchronize()
    raw = got.cpu().numpy().tobytes()
    return b"".join(GF.lem(int.from_bytes(raw[o:o + 32], "little")) for o in range(0, len(raw), 32))


# -- 1. the G2 linear-combination aid -------------------------------------------------------------------------------------------
def _lincomb2(logs, rhos):
    import torch
    d_in = torch.from_numpy(device_canonical(2, logs)).cuda()
    rho = np.frombuffer(b"".join(x.to_bytes(16, "little") for x in rhos), dtype=np.uint8).reshape(len(rhos), 16)
    got = PKG.bn254_g2_lincomb128_device(d_in, torch.from_numpy(rho.copy()).cuda())
    torch.cuda.synchronize()
    assert tuple(got.shape) == (128,)
    return got.cpu().numpy().tobytes()


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257))
def test_g2_lincomb_aid(n):
    """one point; a pair that cancels; a workgroup (one wave) short of one point, full, one more; five workgroups with a last one of
    one point.  From 63 points on the list holds rho = 0, 1 and 2^128 - 1, an infinity point with a nonzero rho, and a pair
    P, P and a pair P, -P with equal rho in two slots that the workgroup's tree adds first (32 apart)."""
    rnd = random.Random(3000 + n)
    top = (1 << 128) - 1
    logs = [rnd.randrange(1, R) for _ in range(n)]
    rhos = [rnd.randrange(1 << 128) for _ in range(n)]
    if n == 1:
        rhos[0] = top
    elif n == 2:
        logs[1], rhos[1] = R - logs[0], rhos[0]
    else:
        rhos[0], rhos[1], rhos[2] = 0, 1, top
        logs[3 + 32], rhos[3 + 32] = logs[3], rhos[3]        # P + P: the doubling branch
        logs[5 + 32], rhos[5 + 32] = R - logs[5], rhos[5]    # P + (-P)
        logs[7] = 0                                          # infinity with a nonzero rho
        rhos[n - 1] = top
    want = device_canonical(2, [sum(r * k for r, k in zip(rhos, logs)) % R]).tobytes()
    assert _lincomb2(logs, rhos) == want
    assert any(want) == (n != 2)


def test_g2_lincomb_aid_zero_rho_and_infinity():
    rnd = random.Random(3100)
    assert _lincomb2([rnd.randrange(1, R) for _ in range(65)], [0] * 65) == bytes(128)
    assert _lincomb2([0] * 65, [rnd.randrange(1, 1 << 128) for _ in range(65)]) == bytes(128)
    logs = [0, 0, 5, 0]
    assert _lincomb2(logs, [9, 8, 7, 6]) == device_canonical(2, [35]).tobytes()


# -- 2. the powers check --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ptau_sections(power, tau=TAU, prepared=False):
    return PF.sections(power, tau, ALPHA, BETA, prepared=prepared, points=device_points)


@functools.lru_cache(maxsize=None)
def ptau(power, tau=TAU, prepared=False):
    return PF.assemble(ptau_sections(power, tau, prepared))


def broken_ptau(power, **changed):
    """the honest file of `power` with the bodies of sections s<id> replaced"""
    secs = dict(ptau_sections(power))
    for k, body in changed.items():
        secs[int(k[1:])] = body
    return PF.assemble(secs)


@pytest.mark.parametrize("power,domain_power", ((2, 1), (4, 3), (9, 8)))
def test_powers_check_accepts(power, domain_power):
    for seed in (SEED, bytes(32), None):
        PKG.ptau_check_powers(ptau(power), domain_power, seed=seed)
    PKG.ptau_check_powers(bytearray(ptau(power)), domain_power)
    if power == 9:
        PKG.ptau_check_powers(ptau(power), 3, seed=SEED)  # a small domain of a large file


def test_powers_check_in_small_pieces(monkeypatch):
    """CWC_CONTRIBUTE_CHUNK = 100: the 511 rho of the domain 2^8 in several pieces per range, the last one short"""
    monkeypatch.setenv("CWC_CONTRIBUTE_CHUNK", "100")
    PKG.ptau_check_powers(ptau(9), 8, seed=SEED)
    s2 = ptau_sections(9)[2]
    with pytest.raises(PKG.WitnessCalcError, match=r"^ptau: section 2 \(tauG1\): the first 2n points"):
        PKG.ptau_check_powers(broken_ptau(9, s2=patched(s2, 64 * 510, s2[64 * 509:64 * 510])), 8, seed=SEED)


def _powers_breaks():
    """{name: (file of power 4, the start of the message at domain power 3)}"""
    s = ptau_sections(4)
    one = lambda group, k: device_points(group, [k])  # noqa: E731
    sec = {2: r"^ptau: section 2 \(tauG1\): the first 2n points are not consecutive powers of the tau of section 3$", 3: r"^ptau: section 3 \(tauG2\): ",
           4: r"^ptau: section 4 \(alphaTauG1\): ", 5: r"^ptau: section 5 \(betaTauG1\): ", 6: r"^ptau: section 6 \(betaG2\): "}
    outside = SF.point_of("g2_plus_torsion", random.Random(11))
    assert GF.G2.on_curve(outside) and not SF.in_g2_by_order(outside)
    other_tau = ptau_sections(4, OTHER)
    return {
        "tauG1_5_plus_one": (broken_ptau(4, s2=patched(s[2], 64 * 5, one(1, pow(TAU, 5, R) + 1))), sec[2]),
        "tauG1_6_7_swapped": (broken_ptau(4, s2=patched(s[2], 64 * 6, s[2][64 * 7:64 * 8] + s[2][64 * 6:64 * 7])), sec[2]),
        "tauG1_last_of_2n": (broken_ptau(4, s2=patched(s[2], 64 * 15, one(1, 3))), sec[2]),
        "tauG2_of_another_tau": (broken_ptau(4, s3=other_tau[3]), sec[2]),  # tauG2[1] is the tau of the first equation
        "tauG2_3_replaced": (broken_ptau(4, s3=patched(s[3], 128 * 3, one(2, pow(TAU, 3, R) + 1))), sec[3]),
        "tauG2_last_of_n": (broken_ptau(4, s3=patched(s[3], 128 * 7, one(2, 3))), sec[3]),
        "alphaTauG1_2_of_another_alpha": (broken_ptau(4, s4=patched(s[4], 64 * 2, one(1, OTHER * pow(TAU, 2, R)))), sec[4]),
        "betaTauG1_2_of_another_beta": (broken_ptau(4, s5=patched(s[5], 64 * 2, one(1, OTHER * pow(TAU, 2, R)))), sec[5]),
        "beta2_of_another_beta": (broken_ptau(4, s6=one(2, OTHER)), sec[6]),
        "tauG2_4_outside_the_subgroup": (broken_ptau(4, s3=patched(s[3], 128 * 4, GF.g2_bytes(outside))),
                                         r"^ptau: section 3 \(tauG2\) point 4 is not in the order-r subgroup of G2$"),
    }


POWERS_BREAKS = ("tauG1_5_plus_one", "tauG1_6_7_swapped", "tauG1_last_of_2n", "tauG2_of_another_tau", "tauG2_3_replaced", "tauG2_last_of_n",
                 "alphaTauG1_2_of_another_alpha", "betaTauG1_2_of_another_beta", "beta2_of_another_beta", "tauG2_4_outside_the_subgroup")


@functools.lru_cache(maxsize=None)
def powers_breaks():
    out = _powers_breaks()
    assert tuple(out) == POWERS_BREAKS
    return out


@pytest.mark.parametrize("name", POWERS_BREAKS)
def test_powers_check_refuses(name):
    file, pattern = powers_breaks()[name]
    for seed in (SEED, SEED, None):  # the same seed gives the same verdict; a drawn one too
        with pytest.raises(PKG.WitnessCalcError, match=pattern):
            PKG.ptau_check_powers(file, 3, seed=seed)


def test_powers_check_stops_at_the_prefixes():
    """tauG1[2n], tauG2[n], alphaTauG1[n] and betaTauG1[n] are not read for the domain n = 2^3: a change there is not seen, and it
    is seen for the domain 2^4 of a larger file's same points"""
    s = ptau_sections(5)
    gen1, gen2 = device_points(1, [3]), device_points(2, [3])
    beyond = broken_ptau(5, s2=patched(s[2], 64 * 16, gen1), s3=patched(s[3], 128 * 8, gen2), s4=patched(s[4], 64 * 8, gen1), s5=patched(s[5], 64 * 8, gen1))
    PKG.ptau_check_powers(beyond, 3, seed=SEED)
    with pytest.raises(PKG.WitnessCalcError, match=r"^ptau: section 2 \(tauG1\)"):
        PKG.ptau_check_powers(beyond, 4, seed=SEED)


# -- 3. keys (the constraint systems of test_gpu_groth16_contribute.py, constructions restated) --------------------------------
def _power_system(p):
    n_pub_in = 0 if p <= 2 else 2
    n_pub = n_pub_in + (0 if p <= 2 else 1)
    n_c = (1 << p) - n_pub - 1 - random.Random(p).randrange(0, 1 << (p - 1))
    rnd = random.Random(100 + p)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(n_c)]
    pl = F.planted_system(rnd, 6, shapes, [1, R - 1, 2, F.MONT_R, None])
    return pl.constraints, pl.n_wires, n_pub - n_pub_in, n_pub_in, p


def _column_edges_system(beta=BETA):
    n_c, n_wires = 10, 9
    rnd = random.Random(42)
    cons = []
    for k in range(n_c):
        a = [(4, rnd.randrange(1, R))]
        b = [(3, rnd.randrange(1, R))] if k % 3 == 0 else [(0, 1)]
        c = [(2, rnd.randrange(1, R))] if k % 4 == 1 else []
        cons.append((a, b, c))
    cons[2][0].append((5, 9))
    cons[2][2].append((5, -beta * 9 % R))               # w_5 = -beta u_5, v_5 = 0: the C point of wire 5 is infinity
    cons[6][0].extend([(6, 3), (8, R - 1), (6, 5)])
    cons[7][1].extend([(7, 12345), (8, 2), (7, R - 12345)])
    return cons, n_wires, 0, 0, 4


SYSTEMS = {"p1": functools.partial(_power_system, 1), "p3": functools.partial(_power_system, 3), "column_edges": _column_edges_system}


@functools.lru_cache(maxsize=None)
def system(name):
    """(domain power, R1cs, its bytes, its constraints, (n_wires, n_pub_out, n_pub_in))"""
    cons, n_wires, n_pub_out, n_pub_in, p = SYSTEMS[name]()
    data = F.write_r1cs(n_wires, cons, n_pub_out=n_pub_out, n_pub_in=n_pub_in)
    r1 = PKG.R1cs(data)
    assert r1.qap_info()["domain_power"] == p
    return p, r1, data, cons, (n_wires, n_pub_out, n_pub_in)


@functools.lru_cache(maxsize=None)
def chain(name):
    """(key0, k1, k2, hash1, hash2): the key of the system and ptau(p + 1) with delta = 1, then two contributions"""
    p, r1 = system(name)[:2]
    k0 = PKG.groth16_setup_ptau(r1, ptau(p + 1), 1, "compute")
    k1, h1 = PKG.groth16_contribute(k0, name="first", delta=D_A)
    k2, h2 = PKG.groth16_contribute(k1, name="second", delta=D_B)
    return k0, k1, k2, h1, h2


def verify(name, key, **kw):
    p, r1 = system(name)[:2]
    kw.setdefault("seed", SEED)
    return PKG.groth16_verify_key(key, r1, kw.pop("file", ptau(p + 1)), **kw)


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_verify_key_accepts_the_chain(name):
    k0, k1, k2, h1, h2 = chain(name)
    assert verify(name, k0) == []
    assert verify(name, k1) == [h1]
    assert verify(name, k2) == [h1, h2] and h1 != h2
    assert verify(name, k2, seed=None, check_ptau=True) == [h1, h2]
    assert verify(name, k2, lagrange="auto", records=False) == [h1, h2]
    ms = PKG.groth16_verify_key_phase_ms()
    assert list(ms) == list(PKG.GROTH16_VERIFY_KEY_PHASES) and all(x > 0 for x in ms.values())
    if name == "column_edges":
        c = sections(k2)[8]
        assert not any(c[64 * 4:64 * 5]) and any(c[64:128])  # the C point of wire 5 is infinity


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_verify_key_with_a_prepared_file(name):
    """lagrange = "file" reads the Lagrange forms of sections 12 to 15: a key made that way and a key made under "compute" hold the
    same bytes, and both verify under "file", "auto" and "compute" """
    p, r1 = system(name)[:2]
    prepared = ptau(p + 1, prepared=True)
    made_file, h = PKG.groth16_contribute(PKG.groth16_setup_ptau(r1, prepared, 1, "file"), name="first", delta=D_A)
    for mode in ("file", "auto", "compute"):
        assert verify(name, made_file, file=prepared, lagrange=mode, check_ptau=(mode == "file")) == [h]
    assert verify(name, chain(name)[1], file=prepared, lagrange="file") == [chain(name)[3]]
    with pytest.raises(PKG.WitnessCalcError, match="^ptau: lagrange = file, but the file has no prepared sections"):
        verify(name, made_file, lagrange="file")


# -- 4. refusals ----------------------------------------------------------------------------------------------------------------
def _c_and_h_tampers():
    """{name: (system, key, the section named)}: keys whose C or H alone was changed; every one is refused with and without the
    records"""
    k2 = chain("p3")[2]
    s = sections(k2)
    gen = GF.g1_bytes(GF.G1_GEN)
    n_c, n_h = len(s[8]) // 64, len(s[9]) // 64
    assert n_c >= 3 and n_h == 8 and all(any(s[8][64 * i:64 * i + 64]) for i in (0, 1, n_c - 1)) and s[8][:64] != s[8][64:128]
    e2 = chain("column_edges")[2]
    se = sections(e2)
    assert not any(se[8][64 * 4:64 * 5])
    moved = patched(patched(s[8], 0, g1_sum(s[8][:64], gen)), 64 * (n_c - 1), g1_sum(s[8][-64:], gen, -1))  # C_0 + P, C_last - P
    return {
        "C_first": ("p3", with_sections(k2, s8=patched(s[8], 0, gen)), "8 (C)"),
        "C_last": ("p3", with_sections(k2, s8=patched(s[8], 64 * (n_c - 1), gen)), "8 (C)"),
        "H_first": ("p3", with_sections(k2, s9=patched(s[9], 0, gen)), "9 (H)"),
        "H_last": ("p3", with_sections(k2, s9=patched(s[9], 64 * (n_h - 1), gen)), "9 (H)"),
        "C_infinity_made_a_point": ("column_edges", with_sections(e2, s8=patched(se[8], 64 * 4, gen)), "8 (C)"),
        "C_point_made_infinity": ("column_edges", with_sections(e2, s8=patched(se[8], 64, bytes(64))), "8 (C)"),
        "C_two_swapped": ("p3", with_sections(k2, s8=patched(s[8], 0, s[8][64:128] + s[8][:64])), "8 (C)"),
        "C_plus_P_and_minus_P": ("p3", with_sections(k2, s8=moved), "8 (C)"),
        "C_all_times_k": ("p3", with_sections(k2, s8=scale_stored(s[8], 3)), "8 (C)"),
        "H_all_times_k": ("p3", with_sections(k2, s9=scale_stored(s[9], R - 1)), "9 (H)"),
    }


TAMPERS = ("C_first", "C_last", "H_first", "H_last", "C_infinity_made_a_point", "C_point_made_infinity", "C_two_swapped", "C_plus_P_and_minus_P",
           "C_all_times_k", "H_all_times_k")


@functools.lru_cache(maxsize=None)
def c_and_h_tampers():
    out = _c_and_h_tampers()
    assert tuple(out) == TAMPERS
    return out


@pytest.mark.parametrize("records", (True, False))
@pytest.mark.parametrize("name", TAMPERS)
def test_verify_key_refuses_a_changed_c_or_h(name, records):
    sysname, key, what = c_and_h_tampers()[name]
    for seed in (SEED, None):
        with pytest.raises(PKG.WitnessCalcError, match="^zkey verify: section %s is not the remade key's section divided by delta$" % what.replace("(", r"\(").replace(")", r"\)")):
            verify(sysname, key, records=records, seed=seed)


def refused(name, key, pattern, **kw):
    with pytest.raises(PKG.WitnessCalcError, match=pattern):
        verify(name, key, **kw)


def test_verify_key_refuses_changed_structure():
    p, r1, _, cons, (n_wires, n_pub_out, n_pub_in) = system("p3")
    k2 = chain("p3")[2]
    s = sections(k2)
    names = {3: "IC", 5: "A", 6: "B1", 7: "B2"}
    for sid, nm in names.items():
        at, twice = doubled(s[sid], 128 if sid == 7 else 64)
        for records in (True, False):
            refused("p3", with_sections(k2, **{"s%d" % sid: patched(s[sid], at, twice)}), r"^zkey verify: section %d \(%s\) differs from %s$" % (sid, nm, REMADE),
                    records=records)
    header = r"^zkey verify: section 2 \(header\) differs from %s before delta1 \(the sizes, alpha1, beta1, beta2 or gamma2\)$" % REMADE
    refused("p3", with_sections(k2, s2=patched(s[2], HDR_ALPHA1, GF.g1_bytes(GF.G1_GEN))), header)
    gamma2 = sections(PKG.groth16_setup(r1, (TAU, ALPHA, BETA, 7, 1)))[2][HDR_GAMMA2:HDR_GAMMA2 + 128]
    assert gamma2 != s[2][HDR_GAMMA2:HDR_GAMMA2 + 128]
    refused("p3", with_sections(k2, s2=patched(s[2], HDR_GAMMA2, gamma2)), header)
    refused("p3", with_sections(k2, s1=struct.pack("<I", 2)), "^zkey")  # not Groth16: the loader's refusal
    # the key of a circuit of the same sizes with one coefficient changed, against the first circuit; and the reverse
    k, side = next((k, side) for k, c in enumerate(cons) for side in (0, 1) if len(c[side]))
    (wire, co), rest = list(F.terms(cons[k][side]))[0], list(F.terms(cons[k][side]))[1:]
    lc = [(wire, (co + 1) % R or 2)] + [(w, c % R) for w, c in rest]
    other_cons = [tuple(lc if (j, sd) == (k, side) else c[sd] for sd in range(3)) for j, c in enumerate(cons)]
    other = PKG.R1cs(F.write_r1cs(n_wires, other_cons, n_pub_out=n_pub_out, n_pub_in=n_pub_in))
    assert other.qap_info()["domain_power"] == p
    other_k1, _ = PKG.groth16_contribute(PKG.groth16_setup_ptau(other, ptau(p + 1), 1, "compute"), delta=D_A)
    assert PKG.groth16_verify_key(other_k1, other, ptau(p + 1)) != []
    coefficient = r"^zkey verify: section 4 differs from the r1cs at constraint \d+, matrix %s, signal %d$" % ("AB"[side], wire)
    refused("p3", other_k1, coefficient)
    with pytest.raises(PKG.WitnessCalcError, match=coefficient):
        PKG.groth16_verify_key(k2, other, ptau(p + 1), records=False)
    # a file of another tau: the first section that depends on the points differs
    refused("p3", k2, r"^zkey verify: section 3 \(IC\) differs from %s$" % REMADE, file=ptau(p + 1, OTHER))
    # a key of other sizes
    assert n_wires != 9
    refused("column_edges", k2, r"^zkey verify: nVars of the key is %d, the circuit's is 9$" % n_wires)


def test_verify_key_refuses_changed_records_and_delta():
    k0, k1, k2, h1, h2 = chain("p3")
    s = sections(k2)
    cs_hash, recs = CF.read_section10(s[10])
    delta1, delta2 = s[2][HDR_DELTA1:HDR_DELTA1 + 64], s[2][HDR_DELTA1 + 64:HDR_DELTA1 + 192]
    # delta1 times k with no record of it: the chain of deltas breaks; without the records delta2 no longer fits
    moved1 = with_sections(k2, s2=patched(s[2], HDR_DELTA1, scale_stored(delta1, 5)))
    refused("p3", moved1, "^zkey verify: delta1 is not the deltaAfter of the last contribution$")
    refused("p3", moved1, "^zkey verify: delta2 is not the G2 generator times delta1's scalar$", records=False)
    # delta1 and delta2 disagreeing
    other2 = GF.g2_bytes(GF.G2.to_affine(GF.G2.mul(g2_of(delta2), 5)))
    for records in (True, False):
        refused("p3", with_sections(k2, s2=patched(s[2], HDR_DELTA1 + 64, other2)), "^zkey verify: delta2 is not the G2 generator times delta1's scalar$", records=records)
    # both moved together, C and H left: every record rule holds but the chain's end, and without the records C no longer fits
    both = with_sections(k2, s2=patched(s[2], HDR_DELTA1, scale_stored(delta1, 5) + other2))
    refused("p3", both, "^zkey verify: delta1 is not the deltaAfter of the last contribution$")
    refused("p3", both, r"^zkey verify: section 8 \(C\) is not the remade key's section divided by delta$", records=False)
    for at, what in ((HDR_DELTA1, "delta1"), (HDR_DELTA1 + 64, "delta2")):
        gone = with_sections(k2, s2=patched(s[2], at, bytes(64 if what == "delta1" else 128)))
        refused("p3", gone, "^zkey verify: %s is the point at infinity$" % what, records=False)
    # csHash altered
    flipped = with_sections(k2, s10=patched(s[10], 5, bytes([s[10][5] ^ 1])))
    refused("p3", flipped, "^zkey verify: section 10: the csHash is not the hash of sections 1 to 9 of the remade key$")
    assert verify("p3", flipped, records=False) == [h1, h2]
    # a record removed: the first, so that the second's transcript no longer fits; the last, so that delta1 has no account
    refused("p3", with_sections(k2, s10=CF.write_section10(cs_hash, recs[1:])), "^zkey verify: contribution 1: the transcript is not that of")
    refused("p3", with_sections(k2, s10=CF.write_section10(cs_hash, recs[:1])), "^zkey verify: delta1 is not the deltaAfter of the last contribution$")
    refused("p3", with_sections(k2, s10=CF.NO_RECORDS), "^zkey verify: delta is not the generator and no contribution accounts for it$")
    assert verify("p3", with_sections(k2, s10=CF.NO_RECORDS), records=False) == []
    # a record's proof of knowledge: g2_spx another multiple of the challenge
    r0 = recs[0]
    forged = CF.Record(r0.delta_after, r0.g1_s, r0.g1_sx, GF.G2.to_affine(GF.G2.mul(r0.g2_spx, 2)), r0.transcript, 0, r0.params)
    refused("p3", with_sections(k2, s10=CF.write_section10(cs_hash, [forged, recs[1]])), "^zkey verify: contribution 1: g1_sx is not g1_s times the secret")
    # the contribution check alone accepts what the key check refuses above: it never saw the circuit
    assert PKG.groth16_verify_contributions(c_and_h_tampers()["C_first"][1]) == [h1, h2]


def test_verify_key_without_records():
    """the trapdoor setup with delta != 1 holds the chain's bytes in sections 1 to 9 and no record: only records=False accepts it"""
    r1 = system("p3")[1]
    trap = PKG.groth16_setup(r1, (TAU, ALPHA, BETA, 1, D_A * D_B % R))
    chained = sections(chain("p3")[2])
    assert all(sections(trap)[i] == chained[i] for i in range(1, 10))
    assert verify("p3", trap, records=False) == []
    refused("p3", trap, "^zkey verify: delta is not the generator and no contribution accounts for it$")
    refused("p3", PKG.groth16_setup(r1, (TAU, ALPHA, BETA, 7, D_A)), r"^zkey verify: section 3 \(IC\) differs", records=False)


def test_check_ptau_is_what_sees_a_broken_power():
    """a key honestly made from a file whose tauG1[5] is another point matches the key remade from that file: only the powers
    check tells"""
    p, r1 = system("p3")[:2]
    s = ptau_sections(p + 1)
    broken = broken_ptau(p + 1, s2=patched(s[2], 64 * 5, device_points(1, [pow(TAU, 5, R) + 1])))
    key, h = PKG.groth16_contribute(PKG.groth16_setup_ptau(r1, broken, 1, "compute"), delta=D_A)
    assert key != chain("p3")[1]
    assert verify("p3", key, file=broken) == [h]
    refused("p3", key, r"^ptau: section 2 \(tauG1\): the first 2n points are not consecutive powers of the tau of section 3$", file=broken, check_ptau=True)
    refused("p3", key, r"^zkey verify: section \d", check_ptau=True)  # against the honest file


# -- 5. the CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_verify_key(tmp_path):
    """groth16-setup --ptau --delta 1, two contributions, --verify-key; every step under its own time limit"""
    p, _, r1cs_bytes = system("p3")[:3]
    (tmp_path / "c.r1cs").write_bytes(r1cs_bytes)
    (tmp_path / "pot.ptau").write_bytes(ptau(p + 1, prepared=True))
    (tmp_path / "one.txt").write_text("1\n")
    path = lambda name: str(tmp_path / name)  # noqa: E731

    def run(tool, *args):
        q = subprocess.run([os.path.join(BIN, tool)] + list(args), capture_output=True, text=True, timeout=120)
        return q.returncode, q.stdout, q.stderr

    assert run("groth16-setup", "--ptau", path("pot.ptau"), "--delta", path("one.txt"), "--lagrange", "compute", path("c.r1cs"), path("k0.zkey"))[0] == 0
    rc, h1, _ = run("groth16-contribute", "--name", "first", path("k0.zkey"), path("k1.zkey"))
    assert rc == 0
    rc, h2, _ = run("groth16-contribute", "--name", "second", path("k1.zkey"), path("k2.zkey"))
    assert rc == 0
    rc, out, err = run("groth16-contribute", "--verify-key", path("c.r1cs"), path("pot.ptau"), path("k2.zkey"))
    assert rc == 0 and out.startswith("OK!") and "2 contributions" in out and out.splitlines()[1:] == [h1.strip(), h2.strip()], (out, err)
    rc, out, err = run("groth16-contribute", "--verify-key", "--lagrange", "file", "--check-ptau", "--skip-records", path("c.r1cs"), path("pot.ptau"), path("k2.zkey"))
    assert rc == 0 and out.startswith("OK!") and "(not verified)" in out, (out, err)
    k2 = (tmp_path / "k2.zkey").read_bytes()
    s = sections(k2)
    (tmp_path / "bad.zkey").write_bytes(with_sections(k2, s9=patched(s[9], 64, GF.g1_bytes(GF.G1_GEN))))
    rc, out, err = run("groth16-contribute", "--verify-key", path("c.r1cs"), path("pot.ptau"), path("bad.zkey"))
    assert rc == 1 and out == "" and err.strip() == "INVALID: zkey verify: section 9 (H) is not the remade key's section divided by delta"
    rc, _, err = run("groth16-contribute", "--verify-key", path("c.r1cs"), path("pot.ptau"), path("missing.zkey"))
    assert rc == 2 and "cannot read" in err
    rc, _, err = run("groth16-contribute", "--verify-key", path("c.r1cs"), path("pot.ptau"), path("c.r1cs"))
    assert rc == 2 and err.startswith("error: zkey")
