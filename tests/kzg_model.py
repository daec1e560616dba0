"""The tiled evaluate-and-quotient recursion of the KZG layer (include/graph_witness_kzg.h, r1cs/kzg.hip) on plain integers: the
specification that the kernels are written against, with no constant taken from the library.

s_i = sum_{j >= i} c_j z^(j-i), so y = p(z) = s_0 and the quotient (p(X) - y) / (X - z) has q_i = s_{i+1}.  A tile of `tile`
consecutive coefficients is `threads` runs of `run` coefficients; a run is folded by Horner, a wave of `wave` runs by a suffix
scan whose step d multiplies by z^(run 2^d), the waves of a tile serially; the tile totals B_b obey K_b = B_(b+1) + z^tile K_(b+1),
which is the same problem on len / tile elements at the point z^tile, and its quotient is K."""
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def horner(c, z):
    """(y, q) by synchronous division: the oracle"""
    s, out = 0, []
    for x in reversed(c):
        s = (x + z * s) % R
        out.append(s)
    out.reverse()  # out[i] = s_i
    return (out[0] if out else 0), out[1:]


def wave_scan(h, m):
    """inclusive suffix scan of the runs' sums h over one wave: x_l = sum_{k >= l} h_k m^(k-l), in log2(len) doubling steps"""
    x, n, d = list(h), len(h), 0
    while (1 << d) < n:
        mult = pow(m, 1 << d, R)
        x = [(x[l] + mult * x[l + (1 << d)]) % R if l + (1 << d) < n else x[l] for l in range(n)]
        d += 1
    return x


def tile_pass(c, z, tile, run, wave, carry):
    """One tile (len(c) <= tile, zero-padded): (B, s) with B the tile's own total and s_i = t_i + z^(tile end - i) carry"""
    n = len(c)
    c = list(c) + [0] * (tile - n)
    threads = tile // run
    assert threads * run == tile and threads % wave == 0
    h = []
    for t in range(threads):
        acc = 0
        for r in reversed(range(run)):
            acc = (c[t * run + r] + z * acc) % R
        h.append(acc)
    zr = pow(z, run, R)
    waves = [wave_scan(h[w:w + wave], zr) for w in range(0, threads, wave)]
    span = pow(zr, wave, R)

    def above(w, k):  # what the waves above w and the carry k add at wave w's end
        for v in reversed(range(w + 1, len(waves))):
            k = (waves[v][0] + span * k) % R
        return k

    total = (waves[0][0] + span * above(0, 0)) % R
    s = [0] * tile
    for w, xs in enumerate(waves):
        k = above(w, carry)
        full = [(xs[l] + pow(zr, wave - l, R) * k) % R for l in range(wave)]
        for l in range(wave):
            acc = full[l + 1] if l + 1 < wave else k
            t = w * wave + l
            for r in reversed(range(run)):
                acc = (c[t * run + r] + z * acc) % R
                s[t * run + r] = acc
    return total, s[:n]


def levels(n, tile):
    """how many levels the recursion has for n coefficients"""
    k = 1
    while n > tile:
        n, k = -(-n // tile), k + 1
    return k


def eval_quotient(c, z, tile, run=None, wave=64):
    """(y, q) through the tiled recursion"""
    c = [x % R for x in c]
    z %= R
    run = run or max(1, tile // 256)
    if not c:
        return 0, []
    tiles = [c[i:i + tile] for i in range(0, len(c), tile)]
    if len(tiles) == 1:
        _, s = tile_pass(c, z, tile, run, wave, 0)
        return s[0], s[1:]
    totals = [tile_pass(t, z, tile, run, wave, 0)[0] for t in tiles]
    _, carries = eval_quotient(totals, pow(z, tile, R), tile, run, wave)
    s = []
    for t, k in zip(tiles, carries + [0]):
        s += tile_pass(t, z, tile, run, wave, k)[1]
    return s[0], s[1:]
