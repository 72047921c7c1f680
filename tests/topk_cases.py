"""Case table and numpy replay shared by tests/test_topk_cases.py (no GPU) and
tests/test_gpu_topk_stages.py (tpe_pool_topk's six kernels, csrc/tpe_pool.hip,
stage by stage).

The replay restates what a call leaves in its scratch (include/tpe_hip.h,
tpe_pool_topk_layout): from (S, taken, k) the control block (T, k_rem, k_eff,
n_less), the tile table's exclusive (less, equal) offsets, the candidate list
-- rows with key < T in row order, then the first k_rem rows with key == T --
and the candidates by (key, row), the output.  It is the reference of the
intermediate state only; the reference of the final order stays the lexsort
rule (test_gpu_pool._expected_order), and test_topk_cases.py holds the replay
to it on every case.

  digit-p       only byte p of the key varies over the untaken rows: pass p of
                the radix select decides alone (a wrong shift or mask there)
  staircase     around one key K, rows that leave K's prefix at every byte, on
                both sides: all eight passes choose among several bins
  ties          T inside a tie class spread over all tiles, 1 <= k_rem <= ties:
                "the first k_rem in row order" (tile_cnt[2t + 1], pe < k_rem,
                n_less + pe); +-0.0 and NaN classes; with and without n_less
  edges         winners at a thread's first / last row, a tile's first / last
                row and the pool's last row; n of 1, 16, 17, 4096, 4097
  rank          k on both sides of k_pool_rank's LDS tiles of 256
  tiles-257/514 258 and 514 tiles: k_pool_scan's threads own 2 and 3 tiles
  none-free     nothing untaken;  k-over: k above the untaken rows

Every builder asserts the property its case is named for.
"""
from collections import namedtuple

import numpy as np

TILE = 4096        # rows per selection tile (tpe_pool_topk_layout reports it)
PER_THREAD = 16    # consecutive rows of a tile that one k_pool_gather thread owns
SCAN_THREADS = 256  # k_pool_scan: one block
RANK_TILE = 256    # candidates k_pool_rank stages in LDS at a time
N3 = 3 * TILE + 17
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)

Case = namedtuple("Case", "name S taken k")
Replay = namedtuple("Replay", "k_eff T mask k_rem n_less tile_off cand_key cand_row out keys")


# -- the replay -------------------------------------------------------------------
def pool_key(s):
    """~order_key (csrc/tpe_common.hpp): a uint64 whose ascending order is the
    rank order.  -0.0 == +0.0, every NaN has key 1 (the smallest there is)."""
    s = np.array(s, np.float64)
    nan = np.isnan(s)
    s[s == 0.0] = 0.0
    b = s.view(np.uint64)
    order = np.where((b >> np.uint64(63)) != 0, ~b, b | np.uint64(1 << 63))
    key = ~order
    key[nan] = 1
    return key


def replay(S, taken, k):
    n = len(S)
    keys = pool_key(S)
    free = np.flatnonzero(np.asarray(taken) == 0)
    fk = keys[free]
    k_eff = min(int(k), n, free.size)
    n_tiles = (n + TILE - 1) // TILE
    tile_off = np.zeros((n_tiles, 2), np.int64)
    none = np.zeros(0, np.int64)
    if k_eff == 0:
        return Replay(0, np.uint64(0), np.uint64(0), 0, 0, tile_off, none.view(np.uint64), none,
                      none, keys)
    T = np.partition(fk, k_eff - 1)[k_eff - 1]
    less, equal = free[fk < T], free[fk == T]
    n_less = int(less.size)
    k_rem = k_eff - n_less
    assert 1 <= k_rem <= equal.size
    for col, rows in enumerate((less, equal)):
        cnt = np.bincount(rows // TILE, minlength=n_tiles)
        tile_off[:, col] = np.cumsum(cnt) - cnt
    cand_row = np.concatenate([less, equal[:k_rem]]).astype(np.int64)
    cand_key = keys[cand_row]
    out = cand_row[np.lexsort((cand_row, cand_key))]
    return Replay(k_eff, T, ALL_ONES, k_rem, n_less, tile_off, cand_key, cand_row, out, keys)


def key_byte(keys, p):
    return ((keys >> np.uint64(8 * (7 - p))) & np.uint64(255)).astype(np.int64)


def from_bits(bits):
    return np.asarray(bits, np.uint64).view(np.float64)


def from_keys(keys):
    """Scores with these keys (not key 1: no score but NaN has it)."""
    order = ~np.asarray(keys, np.uint64)
    top = (order >> np.uint64(63)) != 0
    return from_bits(np.where(top, order & np.uint64((1 << 63) - 1), ~order))


def _taken(rng, n, p=0.3):
    return (rng.uniform(size=n) < p).astype(np.uint8)


# -- digit-p ------------------------------------------------------------------------
DIGIT_K = (1, 100, 257, 5000)


def _digit(p, k):
    rng = np.random.RandomState(4100 + p)
    taken = _taken(rng, N3)
    d = rng.randint(0, 256, N3).astype(np.uint64)
    if p == 0:    # both signs; the exponent field is never 0 and never 0x7FF
        bits = (d << np.uint64(56)) | np.uint64(0x0010000000000000)
    elif p == 1:  # exponents 0x3F0 ... 0x3FF
        bits = np.uint64(0x3F00000000000000) | (d << np.uint64(48))
    else:
        bits = np.uint64(0x3FF0000000000000) | (d << np.uint64(8 * (7 - p)))
    S = from_bits(bits).copy()
    # (a taken row's score is anything: counting one moves every stage)
    S[taken != 0] = rng.normal(size=int(taken.sum()))
    assert np.isfinite(S).all() and (np.abs(S[taken == 0]) >= np.finfo(np.float64).tiny).all()
    fk = pool_key(S)[taken == 0]
    for q in range(8):
        bins = np.unique(key_byte(fk, q)).size
        assert (bins == 1) if q < p else (bins >= 16) if q == p else True, (p, q, bins)
    # ... and the bytes after p are those of the class: byte p alone decides
    assert np.unique(fk).size == np.unique(key_byte(fk, p)).size
    r = replay(S, taken, k)
    assert r.k_eff == k and 0 < r.k_rem and int((fk == r.T).sum()) > 1
    return Case("digit-%d-k%d" % (p, k), S, taken, k)


# -- staircase ------------------------------------------------------------------------
STAIR_K = 0x405566778899AABB  # (the key of the score with bits 0x3FAA998877665544, about 0.052)


def _k_byte(p):
    return (STAIR_K >> (8 * (7 - p))) & 255


def _k_prefix(p):
    """(mask of the bytes above p, K under it)."""
    mask = ((1 << 64) - 1) ^ ((1 << (8 * (8 - p))) - 1)
    return np.uint64(mask), np.uint64(STAIR_K & mask)


def _staircase():
    rng = np.random.RandomState(4200)
    n = N3
    keys = np.zeros(n, np.uint64)
    # fillers: byte 0 differs from K's (0x40); 0x00 / 0xFF (exponent 0x7FF: inf,
    # NaN) and 0x7F / 0x80 (exponent 0: zeros, denormals) are left out
    b0 = rng.choice(np.r_[0x01:0x40, 0x41:0x7F, 0x81:0xFF], n).astype(np.uint64)
    low = rng.randint(0, 1 << 28, n).astype(np.uint64) * np.uint64(1 << 28) + \
        rng.randint(0, 1 << 28, n).astype(np.uint64)
    keys[:] = (b0 << np.uint64(56)) | low
    rows = rng.permutation(n)[:7 * 6 + 3]
    taken = _taken(rng, n)
    taken[rows] = 0
    it = iter(rows)
    for p in range(1, 8):
        shift = 8 * (7 - p)
        for delta in (-3, -2, -1, 1, 2, 3):
            below = int(rng.randint(0, 1 << 30)) & ((1 << shift) - 1)
            digit = (_k_byte(p) + delta) << shift
            keys[next(it)] = np.uint64(int(_k_prefix(p)[1]) | digit | below)
    copies = [next(it) for _ in range(3)]
    keys[copies] = np.uint64(STAIR_K)
    S = from_keys(keys)
    assert np.isfinite(S).all() and np.array_equal(pool_key(S), keys)
    fk = keys[taken == 0]
    for p in range(8):  # several bins inside the surviving prefix, below and above K's digit
        mask, prefix = _k_prefix(p)
        digits = key_byte(fk[(fk & mask) == prefix], p)
        mine = _k_byte(p)
        assert (digits < mine).any() and (digits > mine).any() and (digits == mine).any(), p
    k = int((fk < np.uint64(STAIR_K)).sum()) + 2
    r = replay(S, taken, k)
    assert int(r.T) == STAIR_K and r.k_rem == 2 and int((fk == np.uint64(STAIR_K)).sum()) == 3
    return Case("staircase", S, taken, k)


# -- ties -------------------------------------------------------------------------------
TIE_KINDS = ("plain", "zero", "nan")
TIE_CUTS = ("1", "2", "tile0", "tile0+1", "all-1", "all")
NANS = from_bits([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001,
                  0xFFFFFFFFFFFFFFFF, 0x7FF800000000BEEF])


def _ties(kind, with_hi, cut):
    """hi > mid > lo; a quarter of the rows are mid, in every tile, a third of
    those taken.  A NaN class has nothing before it (key 1), so ``nan`` comes
    without hi rows only; its lo rows include +inf, which NaN precedes."""
    rng = np.random.RandomState(4300 + TIE_KINDS.index(kind))
    n = N3
    cls = rng.choice(3, n, p=[0.15, 0.25, 0.6])  # 0 hi, 1 mid, 2 lo
    taken = _taken(rng, n)
    cls[n - 1], taken[n - 1] = 1, 0  # (the partial tile has its mid row)
    S = np.where(cls == 0, 2.0 + rng.randint(0, 50, n) / 8.0, -1.0 - rng.randint(0, 50, n) / 8.0)
    if kind == "plain":
        S[cls == 1] = 0.75
    elif kind == "zero":
        S[cls == 1] = np.where(rng.uniform(size=int((cls == 1).sum())) < 0.5, 0.0, -0.0)
    else:
        S[cls == 1] = NANS[rng.randint(0, NANS.size, int((cls == 1).sum()))]
        S[np.flatnonzero(cls == 2)[::5]] = np.inf
    if not with_hi:
        taken[cls == 0] = 1   # (their scores stay: a taken row counts nowhere)
    assert kind != "nan" or not with_hi
    mid = np.flatnonzero((cls == 1) & (taken == 0))
    per_tile = np.bincount(mid // TILE, minlength=4)
    assert (per_tile > 0).all() and ((cls == 1) & (taken != 0)).any()
    if kind == "zero":
        assert np.signbit(S[mid]).any() and not np.signbit(S[mid]).all()
    if kind == "nan":
        assert np.unique(S[mid].view(np.uint64)).size == NANS.size
    k_rem = {"1": 1, "2": 2, "tile0": per_tile[0], "tile0+1": per_tile[0] + 1,
             "all-1": mid.size - 1, "all": mid.size}[cut]
    n_hi = int(((cls == 0) & (taken == 0)).sum())
    assert (n_hi > 0) == with_hi
    k = n_hi + int(k_rem)
    r = replay(S, taken, k)
    assert r.T == pool_key(S[mid[:1]])[0] and r.k_rem == k_rem and r.n_less == n_hi
    assert k <= 5000
    return Case("ties-%s-%s-%s" % (kind, "hi" if with_hi else "nohi", cut), S, taken, k)


# -- edges --------------------------------------------------------------------------------
EDGE_N = (1, 16, 17, TILE, TILE + 1, 2 * TILE + 33)


def _edges(n, extra):
    """The winners: a thread's last row and its neighbour's first two (15, 16,
    17), a tile's last row and the next one's first (twice), the last row.
    Their neighbours score higher still and are taken."""
    rng = np.random.RandomState(4400 + n)
    S = np.round(rng.normal(size=n), 2)
    taken = _taken(rng, n)
    win = np.array(sorted({r for r in (15, 16, 17, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, n - 1)
                           if 0 <= r < n}))
    best = np.array(sorted({r for r in (14, 18, TILE - 2, TILE + 1, 2 * TILE - 2, 2 * TILE + 1,
                                        n - 2) if 0 <= r < n} - set(win.tolist())), np.int64)
    S[win] = 10.0 + rng.permutation(win.size)
    taken[win] = 0
    S[best] = 100.0
    taken[best] = 1
    k = win.size + extra
    r = replay(S, taken, k)
    assert set(win.tolist()) <= set(r.out.tolist()) and not set(best.tolist()) & set(r.out.tolist())
    assert r.k_eff == min(k, int((taken == 0).sum()))
    if n > 2 * TILE:
        assert n % TILE and {15, 16, 17, TILE - 1, TILE, n - 1} <= set(win.tolist())
        assert best.size == 7
    return Case("edges-n%d-w%d" % (n, extra), S, taken, k)


# -- rank -----------------------------------------------------------------------------------
RANK_K = (255, 256, 257, 512, 513)


def _rank(k):
    rng = np.random.RandomState(4500)
    S = np.round(rng.normal(size=N3), 1)
    taken = _taken(rng, N3)
    r = replay(S, taken, k)
    assert r.k_eff == k and np.unique(r.cand_key).size < k // 4   # many duplicate keys
    assert not np.array_equal(r.out, r.cand_row)                  # the rank has work to do
    return Case("rank-k%d" % k, S, taken, k)


# -- beyond 256 tiles ---------------------------------------------------------------------------
BIG = {"tiles-257": 257 * TILE + 1, "tiles-514": 513 * TILE + 5}
BIG_K = (1, 64, 1000)


def scan_owner(n_tiles):
    """k_pool_scan's split: (tiles per thread, working threads, tiles of the
    last working thread)."""
    per = -(-n_tiles // SCAN_THREADS)
    working = -(-n_tiles // per)
    return per, working, n_tiles - (working - 1) * per


def _big(name, variant, k):
    """A background of distinct low scores; winners in tile 0, in tiles 255,
    256, 257 and in the last tile, and a few hundred scattered over all tiles
    (so the offsets move from tile to tile).  ``cross``: two tie classes lie
    across the boundary of tiles 255 / 256, and k = 64 and k = 1000 cut them
    there."""
    n = BIG[name]
    n_tiles = -(-n // TILE)
    per, working, last = scan_owner(n_tiles)
    assert (n_tiles, per, working, last) == \
        {"tiles-257": (258, 2, 129, 2), "tiles-514": (514, 3, 172, 1)}[name]
    rng = np.random.RandomState(4600 + n_tiles)
    S = -1.0 - rng.uniform(size=n)
    taken = _taken(rng, n, 0.1)
    a = 256 * TILE
    if variant == "spread":
        for t in (0, 255, 256, 257, n_tiles - 1):
            lo, hi = t * TILE, min(n, (t + 1) * TILE)
            rows = lo + rng.permutation(hi - lo)[:300]
            S[rows] = 1.0 + rng.randint(0, 40, rows.size) / 4.0   # (ties among the winners)
            taken[rows[::2]] = 0
        rows = rng.permutation(n)[:400]
        S[rows] = 1.0 + rng.randint(0, 40, rows.size) / 4.0
        S[n - 1], taken[n - 1] = 50.0, 0     # the pool's last row is the best
        r = replay(S, taken, k)
        assert r.out[0] == n - 1
        tiles = set((r.cand_row // TILE).tolist())
        assert k < 64 or {0, 255, 256, 257, n_tiles - 1} <= tiles
    else:
        hi_rows = rng.permutation(TILE)[:40]
        S[hi_rows] = 10.0 + np.arange(40)
        taken[hi_rows] = 0
        mid = np.arange(a - 25, a + 45)
        S[mid] = 5.0
        taken[mid] = 0
        taken[np.r_[a - 25:a - 20, a + 40:a + 45]] = 1
        mid2 = np.r_[a - 700:a - 25, a + 45:a + 700]
        S[mid2] = 4.0
        scattered = rng.permutation(n)[:400]
        scattered = scattered[(scattered < a - 700) | (scattered >= a + 700)]
        S[scattered] = np.where(S[scattered] > 0.0, S[scattered],
                                1.0 + rng.uniform(size=scattered.size))
        r = replay(S, taken, k)
        assert r.n_less == {1: 0, 64: 40, 1000: 100}[k]
        if k > 1:
            ties = np.flatnonzero((r.keys == r.T) & (taken == 0))
            before = int((ties < a).sum())
            assert 0 < before < r.k_rem < ties.size and (r.cand_row[-1] >= a)
    assert r.k_eff == k
    return Case("%s-%s-k%d" % (name, variant, k), S, taken, k)


# -- nothing to select, and everything -------------------------------------------------------------
def _none_free():
    rng = np.random.RandomState(4700)
    S = rng.normal(size=N3)
    r = replay(S, np.ones(N3, np.uint8), 5)
    assert r.k_eff == 0 and r.out.size == 0
    return Case("none-free", S, np.ones(N3, np.uint8), 5)


def _k_over(which):
    rng = np.random.RandomState(4701)
    n = TILE + 17
    S = np.round(rng.normal(size=n), 1)
    taken = _taken(rng, n)
    free = int((taken == 0).sum())
    k = {"free+7": free + 7, "n+5": n + 5}[which]
    r = replay(S, taken, k)
    assert r.k_eff == free < k and free <= 5000 and r.n_less + r.k_rem == free
    return Case("k-over-%s" % which, S, taken, k)


# -- the table --------------------------------------------------------------------------
def _builders():
    out = []
    for p in range(8):
        for k in DIGIT_K:
            out.append(("digit-%d-k%d" % (p, k), _digit, (p, k)))
    out.append(("staircase", _staircase, ()))
    for kind in TIE_KINDS:
        for with_hi in (True, False):
            if kind == "nan" and with_hi:
                continue
            for cut in TIE_CUTS:
                out.append(("ties-%s-%s-%s" % (kind, "hi" if with_hi else "nohi", cut), _ties,
                            (kind, with_hi, cut)))
    for n in EDGE_N:
        for extra in (0, 2):
            out.append(("edges-n%d-w%d" % (n, extra), _edges, (n, extra)))
    for k in RANK_K:
        out.append(("rank-k%d" % k, _rank, (k,)))
    for name in BIG:
        for variant in ("spread", "cross"):
            for k in BIG_K:
                out.append(("%s-%s-k%d" % (name, variant, k), _big, (name, variant, k)))
    out.append(("none-free", _none_free, ()))
    for which in ("free+7", "n+5"):
        out.append(("k-over-%s" % which, _k_over, (which,)))
    return out


_BUILDERS = _builders()
NAMES = [name for name, _, _ in _BUILDERS]
_LAST = {}


def case(name):
    """The named case, built from its seed (the last one built is kept: the
    large ones are 17 MB each)."""
    if name not in _LAST:
        _LAST.clear()
        fn, args = {n: (f, a) for n, f, a in _BUILDERS}[name]
        c = fn(*args)
        assert c.name == name
        c.S.setflags(write=False)
        c.taken.setflags(write=False)
        _LAST[name] = c
    return _LAST[name]
