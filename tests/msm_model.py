"""Host model of the bookkeeping of the Groth16 prover's multi-scalar multiplication (r1cs/msm.hip), restated from its comments
and code: the shape of an MSM (msm_shape), the signed-digit recoding of a scalar (digits_kernel), the key of an entry, and for
the sorted key list the chunks of K = 32 entries of the accumulation levels (chunks_kernel, run_msm).  No point arithmetic.

Two routes: plain Python integers (raw_windows, digits, keys_of) are the definition; the numpy routes (recode, sorted_entries,
chunk_census) do the same for the lists of tests/test_gpu_groth16_msm.py, up to 2^18 scalars by 17 windows by several rows,
and tests/test_msm_model_host.py holds the two against each other.

The census names, per scalar list, which digit events and which chunk events occur, so that a reader sees which paths of the
kernels a row reaches; the vectors of tests/msm_fixtures.py are built to reach every one of them at every window width."""
import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
K = 32            # entries per accumulation chunk
RED_LANES = 64    # bucket segments per window in reduce_kernel
SIGN = 0x80000000


class Shape:
    def __init__(self, n_sc):
        lg = 0
        while (2 << lg) <= n_sc:
            lg += 1
        self.n_sc = n_sc
        self.c = min(15, max(7, lg - 3 if lg > 3 else 0))
        self.n_win = 254 // self.c + 1
        self.n_b = 1 << (self.c - 1)
        self.per_lane = (self.n_b + RED_LANES - 1) // RED_LANES  # buckets per reduce_kernel lane

    def __repr__(self):
        return "Shape(n_sc=%d, c=%d, n_win=%d, n_b=%d)" % (self.n_sc, self.c, self.n_win, self.n_b)


def msm_shape(n_sc):
    return Shape(n_sc)


def shape_of_c(c):
    """the smallest scalar count with window width c (c = 7: the largest, 2047, is the interesting one)"""
    return Shape(2047 if c == 7 else 1 << (c + 3))


# -- plain integers ------------------------------------------------------------------------------------------------------------
def raw_windows(k, c, n_win):
    """the c bits of k at position c w, for each window (bits_at: positions of 256 and above read as zero)"""
    assert 0 <= k < 1 << 256
    return [(k >> (c * w)) & ((1 << c) - 1) if c * w < 256 else 0 for w in range(n_win)]


def digits(k, c, n_win):
    """canonical k -> n_win signed digits in [-2^(c-1) + 1, 2^(c-1)]; sum d_w 2^(c w) == k"""
    n_b, carry, out = 1 << (c - 1), 0, []
    for raw in raw_windows(k, c, n_win):
        d = raw + carry
        carry = 0
        if d > n_b:
            d -= 2 * n_b
            carry = 1
        out.append(d)
    assert carry == 0, "the top window overflowed: k is not below 2^254"
    return out


def key_of(shape, row, win, d):
    return (row * shape.n_win + win) * shape.n_b + abs(d) - 1


def keys_of(shape, rows):
    """rows of scalars -> [(key, value)] of the nonzero digits in the order digits_kernel writes them (row, window, scalar)"""
    out = []
    for row, scalars in enumerate(rows):
        ds = [digits(k, shape.c, shape.n_win) for k in scalars]
        for win in range(shape.n_win):
            for i, d in enumerate(ds):
                if d[win]:
                    out.append((key_of(shape, row, win, d[win]), i | (SIGN if d[win] < 0 else 0)))
    return out


def level_bounds(n_ent):
    """the list bounds of the levels run_msm launches for n_ent entries: [n_ent, 2 ceil(n_ent / K), ...], the last one <= K"""
    out = [n_ent]
    while out[-1] > K:
        out.append(2 * ((out[-1] + K - 1) // K))
        assert out[-1] < out[-2]
    return out


def straddles(c, win):
    """the window's bits lie in two 32-bit words"""
    return (c * win) % 32 + c > 32 and c * win < 256


# -- numpy ---------------------------------------------------------------------------------------------------------------------
def scalars_array(scalars):
    """ints below 2^256 -> u64 [n, 8] of 32-bit limbs"""
    buf = b"".join(int(k).to_bytes(32, "little") for k in scalars)
    return np.frombuffer(buf, dtype="<u4").reshape(len(scalars), 8).astype(np.uint64)


def recode(limbs, shape):
    """u64 [n, 8] limbs of canonical scalars -> (raw, carry_in, digit), each int32 [n_win, n]"""
    n = limbs.shape[0]
    c, n_b = shape.c, shape.n_b
    ext = np.concatenate([limbs, np.zeros((n, 2), np.uint64)], axis=1)
    raw = np.zeros((shape.n_win, n), np.int32)
    cin = np.zeros((shape.n_win, n), np.int32)
    dig = np.zeros((shape.n_win, n), np.int32)
    carry = np.zeros(n, np.int32)
    for w in range(shape.n_win):
        pos = c * w
        if pos < 256:
            v = (ext[:, pos >> 5] | (ext[:, (pos >> 5) + 1] << np.uint64(32))) >> np.uint64(pos & 31)
            raw[w] = (v & np.uint64((1 << c) - 1)).astype(np.int32)
        cin[w] = carry
        d = raw[w] + carry
        over = d > n_b
        dig[w] = np.where(over, d - 2 * n_b, d)
        carry = over.astype(np.int32)
    assert not carry.any(), "a scalar is not below 2^254"
    return raw, cin, dig


def top_values(shape):
    """(top_max, top_carry): the top window's largest raw value of a scalar below r, and the largest one that a scalar below r
    can have together with a carry in (the carry made by n_b + 1 in the window before the top)"""
    s = shape.c * (shape.n_win - 1)
    top_max = (R - 1) >> s
    for t in (top_max, top_max - 1):
        if (t << s) | ((shape.n_b + 1) << (s - shape.c)) < R:
            return top_max, t
    raise AssertionError


DIGIT_EVENTS = ("top_bucket", "top_bucket_by_carry", "most_negative", "zero_with_carry", "straddle")


def digit_census(shape, raw, cin, dig):
    """-> dict: for each event of DIGIT_EVENTS the sorted windows where it occurs; 'carry_chain', 'top_max', 'top_max_carry',
    'zero_scalar': counts of scalars; 'negative', 'entries': counts of digits"""
    c, n_b, n_win = shape.c, shape.n_b, shape.n_win
    top_max, top_carry = top_values(shape)

    def wins(mask):
        return [int(w) for w in np.nonzero(mask.any(axis=1))[0]]

    out = {"top_bucket": wins((raw == n_b) & (cin == 0)),                  # digit +n_b
           "top_bucket_by_carry": wins((raw == n_b - 1) & (cin == 1)),     # digit +n_b
           "most_negative": wins((raw == n_b + 1) & (cin == 0)),           # digit -(n_b - 1), carry out
           "zero_with_carry": wins((raw == 2 * n_b - 1) & (cin == 1))}     # digit 0 (a sentinel entry), carry out
    st = []
    for w in range(n_win):
        if straddles(c, w):
            low = 32 - (c * w) % 32  # bits of the window in the lower word
            if (((raw[w] & ((1 << low) - 1)) != 0) & ((raw[w] >> low) != 0)).any():
                st.append(w)
    out["straddle"] = st
    out["carry_chain"] = int(cin[1:].all(axis=0).sum())
    out["top_max"] = int(((raw[-1] == top_max) & (cin[-1] == 0)).sum())
    out["top_max_carry"] = int(((raw[-1] == top_carry) & (cin[-1] == 1)).sum())
    out["zero_scalar"] = int((~raw.any(axis=0)).sum())
    out["negative"] = int((dig < 0).sum())
    out["entries"] = int((dig != 0).sum())
    return out


def sorted_entries(shape, digs):
    """[digit array int32 [n_win, n_sc]] (recode's, one per row of the call) -> (keys, vals) of the nonzero digits, u32, stably
    sorted by key as the prover's radix sort leaves them; the sentinel entries (zero digits) that follow them are not listed.
    (Keys grow with (row, window), so each window's entries are sorted by bucket on their own.)"""
    ks, vs = [], []
    idx = np.arange(shape.n_sc, dtype=np.uint32)
    for row, dig in enumerate(digs):
        assert dig.shape == (shape.n_win, shape.n_sc)
        for w in range(shape.n_win):
            d = dig[w]
            nz = np.nonzero(d)[0]
            mag = np.abs(d[nz]).astype(np.uint32)
            order = np.argsort(mag, kind="stable")
            ks.append((np.uint32((row * shape.n_win + w) * shape.n_b) + mag - np.uint32(1))[order])
            vs.append((idx[nz] | np.where(d[nz] < 0, np.uint32(SIGN), np.uint32(0)))[order])
    return np.concatenate(ks), np.concatenate(vs)


CHUNK_EVENTS = ("run_ends_on_seam", "run_starts_on_seam", "run_over_3_chunks", "head_and_tail_partial", "head_then_complete")


def _level(keys):
    """one level over the sorted live keys (the sentinels behind them never match): (events, the next level's keys)"""
    m = keys.size
    n_ch = (m + K - 1) // K
    new = np.ones(m, bool)
    new[1:] = keys[1:] != keys[:-1]                      # entry j starts a run
    starts = np.nonzero(new)[0]
    ends = np.append(starts[1:], m)                      # exclusive
    ev = {"run_ends_on_seam": int(((ends % K == 0) & (ends - starts > 1)).sum()),
          "run_starts_on_seam": int(((starts % K == 0) & (ends - starts > 1)).sum()),
          "run_over_3_chunks": int((ends // K - (starts + K - 1) // K >= 3).sum())}
    first = np.arange(n_ch) * K
    last = np.minimum(first + K, m) - 1
    head = ~new[first]                                   # head_span: the entry before the chunk has the chunk's first key
    tail = np.zeros(n_ch, bool)
    tail[:-1] = ~new[first[1:]]                          # tail_span: the entry behind the chunk has its last key
    one_run = keys[first] == keys[last]
    pad = np.zeros(n_ch * K, bool)
    pad[:m] = new
    runs = pad.reshape(n_ch, K).sum(axis=1) + head       # runs that touch the chunk
    head_partial = head
    tail_partial = tail & ~(head & one_run)              # a chunk inside one long run leaves its head partial only
    ev["head_and_tail_partial"] = int((head_partial & tail_partial).sum())
    ev["head_then_complete"] = int((head & ~one_run & (runs - tail_partial >= 2)).sum())
    ev["partials"] = int(head_partial.sum() + tail_partial.sum())
    ev["entries"], ev["chunks"] = int(m), int(n_ch)
    slots = np.stack([keys[first], keys[last]], axis=1).reshape(-1)
    flags = np.stack([head_partial, tail_partial], axis=1).reshape(-1)
    return ev, slots[flags]


def chunk_census(keys, n_ent):
    """sorted live keys of a call and its entry count (sentinels included) -> {'levels': [events per level that holds
    entries], 'launches': levels run_msm launches}.  The levels follow run_msm: level l + 1 reads the partials of level l."""
    bounds = level_bounds(n_ent)
    levels = []
    for lv in range(len(bounds)):
        if keys.size == 0:
            break
        assert keys.size <= bounds[lv]
        ev, keys = _level(keys)
        levels.append(ev)
    assert keys.size == 0, "the last level left partials"
    return {"levels": levels, "launches": len(bounds)}


def outside_runs(keys, vals, lo, hi):
    """runs whose entries all name scalars outside [lo, hi): their buckets stay the point at infinity in that MSM"""
    idx = vals & np.uint32(SIGN - 1)
    inside = (idx >= lo) & (idx < hi)
    new = np.ones(keys.size, bool)
    new[1:] = keys[1:] != keys[:-1]
    run_id = np.cumsum(new) - 1
    has_inside = np.zeros(run_id[-1] + 1, bool)
    has_inside[run_id[inside]] = True
    return int((~has_inside).sum())


def pair_runs(keys, vals, period):
    """(cancelling, doubling): buckets that hold exactly two entries, of scalars i and i + period, with signs + - and + +"""
    new = np.ones(keys.size, bool)
    new[1:] = keys[1:] != keys[:-1]
    starts = np.nonzero(new)[0]
    ends = np.append(starts[1:], keys.size)
    two = starts[ends - starts == 2]
    a, b = vals[two], vals[two + 1]
    pair = ((a & np.uint32(SIGN)) == 0) & ((b & np.uint32(SIGN - 1)) == a + np.uint32(period))
    return int((pair & ((b & np.uint32(SIGN)) != 0)).sum()), int((pair & ((b & np.uint32(SIGN)) == 0)).sum())


def call_census(shape, lists, lo=0, hi=0):
    """scalar lists (ints) of one prover call -> {'digits': [digit_census per row], 'chunks': chunk_census, 'outside':
    outside_runs for [lo, hi), 'keys', 'vals'}"""
    digs, per_row = [], []
    for scalars in lists:
        raw, cin, dig = recode(scalars_array(scalars), shape)
        per_row.append(digit_census(shape, raw, cin, dig))
        digs.append(dig)
    keys, vals = sorted_entries(shape, digs)
    return {"digits": per_row, "chunks": chunk_census(keys, len(lists) * shape.n_win * shape.n_sc),
            "outside": outside_runs(keys, vals, lo, hi) if hi > lo else 0, "keys": keys, "vals": vals}
