"""Proving from the zkey alone on an MI355X: the witness map of section 4 (r1cs/qap.hip, gwb_zkey_qap_*) against
the `.r1cs` path and the big-integer reference (tests/qap_reference.py), and zkey-only proofs against known discrete logs and the
`.r1cs` path's bytes.  Section 4 is written from plain integers by tests/zkey_coefs_fixtures.py (c R^2 mod r), independent of
r1cs/setup.hip; one test reads a key that setup.hip wrote instead.  Witness-map tests use zkeys whose points are all at infinity
(the loader takes them, and the map does not read them)."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import cwc_import
from tests import groth16_fixtures as GF
from tests import qap_reference as QR
from tests import r1cs_fixtures as F
from tests import zkey_coefs_fixtures as ZF

PKG = cwc_import.load()
R = F.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL = [1, R - 1, 2, F.MONT_R, None]

pytestmark = pytest.mark.gpu


def _planted(seed, n_constraints, n_free=6):
    rnd = random.Random(seed)
    shapes = [{"a": rnd.randrange(0, 4), "b": rnd.randrange(0, 4), "c": rnd.randrange(0, 3)} for _ in range(n_constraints)]
    return F.planted_system(rnd, n_free, shapes, POOL)


def _hollow(n_vars, n_pub, n, entries):
    """a zkey-only Groth16 of the given sizes with every point at infinity and the given section 4 (its bytes: .zkey_bytes)"""
    z = GF.write_zkey(n_vars, n_pub, n, None, None, None, None, None, None, [None] * (n_pub + 1), [None] * n_vars, [None] * n_vars,
                      [None] * n_vars, [None] * (n_vars - n_pub - 1), [None] * n)
    data = ZF.splice(z, ZF.section4(entries))
    g = PKG.Groth16(data)
    g.zkey_bytes = data
    return g


def _map_pair(seed, n_constraints, n_pub_out=1, n_pub_in=2, shuffle=True):
    """planted system -> (planted, R1cs, zkey-only Groth16 over a hollow key, nPub)"""
    pl = _planted(seed, n_constraints)
    n_pub = n_pub_out + n_pub_in
    r1 = PKG.R1cs(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=n_pub_out, n_pub_in=n_pub_in))
    ent = ZF.entries_of(pl.constraints, n_pub)
    if shuffle:
        random.Random(seed).shuffle(ent)
    g = _hollow(pl.n_wires, n_pub, r1.qap_info()["domain_size"], ent)
    g.check_r1cs(r1)
    return pl, r1, g, n_pub


def _h_bytes(constraints, n_pub, rows):
    return np.stack([QR.h_bytes(QR.h_of(constraints, n_pub, w)) for w in rows])


def _device(g, rows_arr, **kw):
    import torch
    out = g.qap_batch_device(torch.from_numpy(rows_arr).cuda(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("full", [False, True], ids=["n_used<n", "n_used==n"])
@pytest.mark.parametrize("p", range(1, 11))
def test_witness_map_domain_powers(p, full):
    """domain 2^p with rows left over, and with nC + nPublic + 1 == 2^p exactly (no padding launch)"""
    n_pub_in = 0 if p <= 2 else 2
    n_pub = n_pub_in + (0 if p <= 2 else 1)
    n = 1 << p
    n_c = n - n_pub - 1 - (0 if full else 1 + random.Random(p).randrange(0, max(1, n // 2 - n_pub - 1)))
    pl, r1, g, _ = _map_pair(200 + p, n_c, n_pub_out=n_pub - n_pub_in, n_pub_in=n_pub_in)
    qi = g.qap_info()
    assert qi["domain_size"] == n == r1.qap_info()["domain_size"] and qi["n_rows"] == n_c + n_pub + 1
    assert (qi["n_rows"] == n) == full
    rnd = random.Random(p)
    rows = [pl.complete(rnd) for _ in range(3)]
    arr = F.rows_array(rows)
    got = g.qap_batch(arr)
    assert np.array_equal(got, r1.qap_batch(arr))
    assert np.array_equal(got, _h_bytes(pl.constraints, n_pub, rows))


@pytest.fixture(scope="module")
def forms_case():
    pl, r1, g, n_pub = _map_pair(41, 40)
    rnd = random.Random(42)
    rows = [pl.complete(rnd) for _ in range(70)]
    return pl, r1, g, rows, _h_bytes(pl.constraints, n_pub, rows)


@pytest.mark.parametrize("batch", [0, 1, 3, 70])
def test_witness_map_batches_and_forms(forms_case, batch):
    pl, r1, g, rows, want = forms_case
    rows, want = rows[:batch], want[:batch]
    arr = F.rows_array(rows) if batch else np.zeros((0, pl.n_wires, 32), np.uint8)
    want_m = F.rows_array([[F.to_montgomery(int.from_bytes(bytes(x), "little")) for x in h] for h in want]) if batch else want
    got = g.qap_batch(arr)
    assert got.shape == (batch, 64, 32) and np.array_equal(got, want) and np.array_equal(got, r1.qap_batch(arr))
    assert np.array_equal(g.qap_batch(arr, montgomery_out=True), want_m)
    assert np.array_equal(_device(g, arr), want)
    assert np.array_equal(_device(g, arr, montgomery_out=True), want_m)
    if batch:
        mont = F.rows_array([[F.to_montgomery(x) for x in w] for w in rows])
        assert np.array_equal(_device(g, mont, montgomery=True), want)
        assert np.array_equal(_device(g, mont, montgomery=True, montgomery_out=True), want_m)


def test_witness_map_rows_above_r(forms_case):
    """elements >= r are reduced mod r, in canonical and in Montgomery rows"""
    pl, r1, g, rows, want = forms_case
    rows, want = rows[:3], want[:3]
    above = [[x + R if x + R < (1 << 256) and i % 3 == 1 else x for i, x in enumerate(w)] for w in rows]
    assert any(x >= R for w in above for x in w)
    assert np.array_equal(_device(g, F.rows_array(above)), want)
    assert np.array_equal(g.qap_batch(F.rows_array(above)), want)
    mont = [[F.to_montgomery(x) for x in w] for w in rows]
    mabove = [[x + R if x + R < (1 << 256) and i % 2 else x for i, x in enumerate(w)] for w in mont]
    assert any(x >= R for w in mabove for x in w)
    assert np.array_equal(_device(g, F.rows_array(mabove), montgomery=True), want)
    assert np.array_equal(_device(g, F.rows_array(mabove)), r1.qap_batch_device(_cuda(F.rows_array(mabove))).cpu().numpy())


def _cuda(arr):
    import torch
    return torch.from_numpy(arr).cuda()


@pytest.fixture(scope="module")
def tile_case():
    """37 + 3 + 1 = 41 rows used: no multiple of 64 / T for any T below 64"""
    pl, r1, g, n_pub = _map_pair(43, 37)
    assert g.qap_info()["n_rows"] == 41
    rnd = random.Random(44)
    rows = [pl.complete(rnd) for _ in range(65)]
    return g, rows, _h_bytes(pl.constraints, n_pub, rows)


@pytest.mark.parametrize("t", [1, 2, 4, 8, 16, 32, 64])
def test_witness_map_every_tile_width(tile_case, t):
    """a batch of T + 1 rows (no multiple of T; two blocks) at every tile width, and the width chosen from the batch"""
    g, rows, want = tile_case
    arr = F.rows_array(rows[:t + 1])
    g.set_tile_width(t)
    try:
        assert np.array_equal(g.qap_batch(arr), want[:t + 1])
        mont = F.rows_array([[F.to_montgomery(x) for x in w] for w in rows[:t + 1]])
        assert np.array_equal(_device(g, mont, montgomery=True), want[:t + 1])
    finally:
        g.set_tile_width(0)
    assert np.array_equal(g.qap_batch(arr), want[:t + 1])


def test_witness_map_row_shape_edges():
    """one hand-made section 4 over a domain of 128: A and B of lengths 0 to 9 and 65 (the unroll-by-4 remainders), A empty with B
    non-empty and the reverse, an interior row without entries, a row of zero values only, an entry at constraint domainSize - 1,
    duplicates, zero values, shuffled order, and the coefficient pool of the check's edge tests.  Reference: the sums as integers."""
    rnd = random.Random(45)
    n, n_vars = 128, 23
    pool = [0, 1, R - 1, 2, R - 2, (R + 1) // 2, F.MONT_R, F.MONT_R_INV, F.MONT_R2, (1 << 255) % R, None]

    def coef():
        c = rnd.choice(pool)
        return rnd.randrange(R) if c is None else c

    lengths = list(range(10)) + [65]
    ent = []
    for i, la in enumerate(lengths):
        lb = lengths[(i + 4) % len(lengths)]
        ent += [(0, i, rnd.randrange(n_vars), coef()) for _ in range(la)]
        ent += [(1, i, rnd.randrange(n_vars), coef()) for _ in range(lb)]
    ent += [(0, 11, s, coef()) for s in (0, 5, n_vars - 1)]                      # B empty
    # row 12: no entry; row 13: zero values only
    ent += [(0, 13, 3, 0), (1, 13, 4, 0)]
    for k, c in enumerate(pool[:-1]):                                           # every pool value on both sides of known rows
        ent += [(0, 14 + k, k + 1, c), (1, 14 + k, n_vars - 1 - k, c)]
    ent += [(0, n - 1, n_vars - 1, R - 1), (1, n - 1, 0, 7)]                    # the last row of the domain
    ent += [(0, 40, 2, 5), (0, 40, 2, R - 5), (0, 40, 2, 9), (1, 40, 6, 1), (1, 40, 6, 1), (1, 40, 6, R - 1)]  # duplicates
    ent += [(m, c, s, 0) for m, c, s, _ in rnd.sample(ent, 12)]                 # zero-valued twins
    assert all(any(e[1] == c for e in ent) for c in (0, 11, 13, n - 1)) and not any(e[1] == 12 for e in ent)
    rnd.shuffle(ent)
    g = _hollow(n_vars, 0, n, ent)
    assert g.qap_info()["n_rows"] == n
    rows = [[1] + [rnd.randrange(R) for _ in range(n_vars - 1)] for _ in range(5)]
    rows[1] = [1] + [R - 1] * (n_vars - 1)
    rows[2] = [1] + [0] * (n_vars - 1)
    want = []
    for w in rows:
        a, b = [0] * n, [0] * n
        for m, c, s, v in ent:
            (b if m else a)[c] = ((b if m else a)[c] + v * w[s]) % R
        want.append(QR.h_bytes(QR.h_ntt(a, b, [x * y % R for x, y in zip(a, b)])))
    want = np.stack(want)
    arr = F.rows_array(rows)
    for t in (0, 1, 64):
        g.set_tile_width(t)
        assert np.array_equal(g.qap_batch(arr), want), t
    mont = F.rows_array([[F.to_montgomery(x) for x in w] for w in rows])
    assert np.array_equal(_device(g, mont, montgomery=True), want)


# -- proofs -------------------------------------------------------------------------------------------------------------------
def _system(seed, n_constraints, n_pub_out=1, n_pub_in=2):
    """planted system -> (planted, R1cs, Trapdoor, zkey bytes with the section 4 of the system)"""
    pl = _planted(seed, n_constraints)
    n_pub = n_pub_out + n_pub_in
    r1 = PKG.R1cs(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=n_pub_out, n_pub_in=n_pub_in))
    T = GF.Trapdoor(pl.constraints, pl.n_wires, n_pub, seed=seed)
    ent = ZF.entries_of(pl.constraints, n_pub)
    random.Random(seed).shuffle(ent)
    return pl, r1, T, ZF.zkey_of(T, ent)


def _want(T, rows, rs):
    return T.want_bytes([T.proof_logs(w, r_, s_) for w, (r_, s_) in zip(rows, rs)])


def _rs(rnd, b):
    return [(rnd.randrange(R), rnd.randrange(R)) for _ in range(b)]


def test_proofs_equal_known_logs_and_the_r1cs_path():
    """host rows, device rows (both forms) and a .wtns image: the zkey alone, the zkey with its R1cs, and the known logs agree"""
    import torch
    pl, r1, T, zkey = _system(51, 40)
    g, g2 = PKG.Groth16(zkey), PKG.Groth16(zkey, r1)
    rnd = random.Random(52)
    rows = [pl.complete(rnd) for _ in range(5)]
    rs = _rs(rnd, 5)
    want = _want(T, rows, rs)
    arr = F.rows_array(rows)
    assert np.array_equal(g.prove_batch(arr, rs=rs), want)
    assert np.array_equal(g2.prove_batch(arr, rs=rs), want)
    d = g.prove_batch_device(torch.from_numpy(arr).cuda(), rs=rs)
    mont = F.rows_array([[F.to_montgomery(x) for x in w] for w in rows])
    dm = g.prove_batch_device(torch.from_numpy(mont).cuda(), rs=rs, montgomery=True)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), want) and np.array_equal(dm.cpu().numpy(), want)
    img = ZF.wtns_image(rows[0])
    proof, public = g.prove_wtns(img, rs=rs[:1])
    assert proof == PKG.proof_json(want[0]) and (proof, public) == g2.prove_wtns(img, rs=rs[:1])
    assert public == [str(x) for x in rows[0][1:T.n_pub + 1]]
    for w, (r_, s_) in zip(rows, rs):
        assert T.verifies(w, *T.proof_logs(w, r_, s_))
    # refusals of the zkey-only calls: a witness of another size, a .wtns image of another size
    with pytest.raises(PKG.WitnessCalcError, match="nVars"):
        g.prove_batch(F.rows_array([rows[0][:-1]]), rs=rs[:1])
    with pytest.raises(PKG.WitnessCalcError, match="nVars"):
        g.prove_wtns(ZF.wtns_image(rows[0] + [0]), rs=rs[:1])
    with pytest.raises(PKG.WitnessCalcError, match="not below r"):
        g.prove_wtns(ZF.wtns_image(rows[0][:-1] + [R]), rs=rs[:1])
    assert g.prove_batch(np.zeros((0, pl.n_wires, 32), np.uint8)).shape == (0, 256)


def test_key_written_by_setup_proves_without_the_r1cs():
    """the writer of section 4 (r1cs/setup.hip) against this reader: a key made by groth16_setup and loaded alone proves rows that
    verify, with the bytes of the `.r1cs` path; a domain with rows left over and one filled exactly"""
    for seed, n_c in ((53, 50), (54, 60)):  # 50 + 4 rows of 64; 60 + 4 = 64
        pl = _planted(seed, n_c)
        r1 = PKG.R1cs(F.write_r1cs(pl.n_wires, pl.constraints, n_pub_out=1, n_pub_in=2))
        trap = tuple(random.Random(seed).randrange(2, R) for _ in range(5))
        zkey = PKG.groth16_setup(r1, trap)
        g, g2 = PKG.Groth16(zkey), PKG.Groth16(zkey, r1)
        g.check_r1cs(r1)
        assert g.qap_info()["n_rows"] == n_c + 4 and g.info["domain_size"] == 64
        rnd = random.Random(seed + 100)
        rows = [pl.complete(rnd) for _ in range(6)]
        rs = _rs(rnd, 6)
        arr = F.rows_array(rows)
        proofs = g.prove_batch(arr, rs=rs)
        assert np.array_equal(proofs, g2.prove_batch(arr, rs=rs))
        assert np.array_equal(g.qap_batch(arr), r1.qap_batch(arr))
        assert list(g.verifying_key().verify_batch(proofs, [w[1:4] for w in rows])) == [PKG.VERIFY_VALID] * 6
        assert list(g.verifying_key().verify_batch(g.prove_batch(arr), [w[1:4] for w in rows])) == [PKG.VERIFY_VALID] * 6


def test_sub_batches_under_small_caps(tmp_path):
    """both workspace caps are read once per process: a child with 1 MiB each proves 9 rows of a small key in sub-batches of the
    prover's workspace, and maps 9 rows over a domain of 2^11 (128 KiB of A / B per row: 8 rows per sub-batch)"""
    pl, r1, T, zkey = _system(55, 30)
    rnd = random.Random(56)
    rows = [pl.complete(rnd) for _ in range(9)]
    rs = _rs(rnd, 9)
    big, big_r1, big_g, _ = _map_pair(57, 2040)
    assert big_g.qap_info()["workspace_bytes_per_row"] == 128 << 10
    big_rows = F.rows_array([big.complete(rnd) for _ in range(9)])
    (tmp_path / "c.zkey").write_bytes(zkey)
    (tmp_path / "big.zkey").write_bytes(big_g.zkey_bytes)
    np.save(tmp_path / "rows.npy", F.rows_array(rows))
    np.save(tmp_path / "big_rows.npy", big_rows)
    (tmp_path / "rs.json").write_text(json.dumps([[str(a), str(b)] for a, b in rs]))
    code = ("import sys, json, numpy as np; sys.path.insert(0, %r); import cwc_import; P = cwc_import.load(); d = %r\n"
            "g = P.Groth16(open(d + '/c.zkey', 'rb').read())\n"
            "rs = [(int(a), int(b)) for a, b in json.load(open(d + '/rs.json'))]\n"
            "np.save(d + '/out.npy', g.prove_batch(np.load(d + '/rows.npy'), rs=rs))\n"
            "b = P.Groth16(open(d + '/big.zkey', 'rb').read())\n"
            "np.save(d + '/big_h.npy', b.qap_batch(np.load(d + '/big_rows.npy')))\n") % (ROOT, str(tmp_path))
    env = dict(os.environ, CWC_GROTH16_WORKSPACE_MB="1", CWC_R1CS_QAP_WORKSPACE_MB="1")
    subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=300)
    assert np.array_equal(np.load(tmp_path / "out.npy"), _want(T, rows, rs))
    assert np.array_equal(np.load(tmp_path / "big_h.npy"), big_r1.qap_batch(big_rows))


def test_cli_four_arguments(tmp_path):
    """groth16-prove circuit.zkey witness.wtns proof.json public.json: the proof verifies, public.json is the witness's signals"""
    pl, r1, T, zkey = _system(58, 35)
    w = pl.complete(random.Random(59))
    (tmp_path / "c.zkey").write_bytes(zkey)
    (tmp_path / "w.wtns").write_bytes(ZF.wtns_image(w))
    cli = os.path.join(ROOT, "circom-witnesscalc_amd", "groth16-prove")
    subprocess.run([cli, str(tmp_path / "c.zkey"), str(tmp_path / "w.wtns"), str(tmp_path / "p.json"), str(tmp_path / "pub.json")],
                   check=True, timeout=300)
    proof = json.loads((tmp_path / "p.json").read_text())
    public = json.loads((tmp_path / "pub.json").read_text())
    assert public == [str(x) for x in w[1:T.n_pub + 1]]
    assert proof["protocol"] == "groth16" and proof["curve"] == "bn128"
    vk = PKG.Groth16VerifyingKey.from_zkey(zkey)
    assert vk.verify(proof, public)
    assert not vk.verify(proof, [public[0], str((int(public[1]) + 1) % R), public[2]])


def test_authv2_class_chain_from_the_zkey_alone():
    """the authV2-class size (2^17 domain), key made on the device by groth16_setup: calc_witness_batch_device and the zkey-only
    prove_batch_device on one stream, three rows; the `.r1cs` path's bytes, and VALID through the pairing"""
    import torch
    C = PKG.graphgen.circuits
    with F.gadget_constraints():
        b = C.build_authv2_class()
    cons = F.derive_r1cs(b)
    gr = PKG.Graph(b.to_bin())
    n_pub = 3
    r1 = PKG.R1cs(F.write_r1cs(len(b._witness), cons, n_pub_in=n_pub))
    zkey = PKG.groth16_setup(r1, (0x1234567 << 200 | 5, 7 << 180 | 11, 13 << 190 | 17, 19 << 170 | 23, 29 << 210 | 31))
    g, g2 = PKG.Groth16(zkey), PKG.Groth16(zkey, r1)
    assert g.info["domain_size"] == 1 << 17
    from tools.synth import synth_inputs
    batch = 3
    rs = _rs(random.Random(60), batch)
    d_in = torch.from_numpy(synth_inputs("field", gr.n_inputs, batch, 43)).cuda()
    d_w = torch.empty((batch, gr.n_witness, 32), dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(batch, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gr.calc_witness_batch_device(d_in, d_w, d_st, stream=s)
        d_p = g.prove_batch_device(d_w, stream=s, rs=rs)
        d_p2 = g2.prove_batch_device(d_w, stream=s, rs=rs)
        st = g.verifying_key().verify_batch_device(d_p, d_w[:, 1:n_pub + 1, :].contiguous(), stream=s)
    s.synchronize()
    assert not d_st.cpu().numpy().any()
    assert np.array_equal(d_p.cpu().numpy(), d_p2.cpu().numpy())
    assert list(st.cpu().numpy()) == [PKG.VERIFY_VALID] * batch
