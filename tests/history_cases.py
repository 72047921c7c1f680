"""Case tables and plain numpy restatements shared by tests/test_history_cases.py
(no GPU) and tests/test_gpu_history_stages.py: the resident history stage by
stage -- tpe_history_append, tpe_history_order, tpe_fit_sorted, tpe_gather_obs
and tpe_gather_obs_multi (csrc/tpe_history.hip, csrc/tpe_sorted.hip).

Nothing here runs a kernel.  The chunk, pass and new-row sizes come from the
host-only tpe_fit_sorted_layout, and a case "at an edge" is edge - 1, edge and
edge + 1 of what it reports.

  append   a scatter: stage (n_labels x k values, then n_labels x k flags) into
           rows [r0, r0 + k) of every column.
  order    np.argsort(key, kind="stable") of a column, key = v or
           log(max(v, floor)): NaN last, -0.0 == +0.0, ties in row order.
           merge_step restates the documented merge rule (an old entry moves by
           the count of new keys below it, a new one by the count of old keys
           at or below it) on dense integer ranks of the keys.
  fit      fit_replay: what tpe_fit_sorted leaves in its scratch -- per
           (segment, chunk) the members in the chunk of rows, how many lie below
           the prior mean, the first member row, the members in the chunk of the
           sorted order; per (segment, row) the rank among the chunk's members --
           and the mixture assembled from those words as csrc/tpe_sorted.hip
           documents it.  test_history_cases.py holds that mixture to
           oracle.adaptive_parzen_normal on the lists oracle.ap_split_trials
           gives, which stays the reference of the final values.
  gather   a loop over positions: position i reads row rows[i] (i without a row
           list), takes it if the row is active for the column and is_below[i]
           is the descriptor's side, in position order; to_int gives
           int(v) - offset.

In every log column any two clamped values are bit-equal or at least 1e-9
apart (relative): the device's log and numpy's may differ in the last bit (one
ulp of a log of magnitude <= 10 is under 2e-15), and the order is defined by
the reference only where that cannot matter (log_separation).
"""
import ctypes
import functools
from collections import namedtuple

import numpy as np

INT32_MAX = 2 ** 31 - 1
IDENT, LOG = 0, 1   # TPE_OBS_IDENTITY, TPE_OBS_LOG
GMM1, LGMM1 = 0, 1  # TPE_GMM1, TPE_LGMM1


def layout(n_seg, n_rows):
    """The nine numbers of tpe_fit_sorted_layout (host only, no GPU)."""
    from hyperopt_amd import _lib as L
    out = (ctypes.c_int64 * 9)()
    got = L.load().tpe_fit_sorted_layout(n_seg, n_rows, ctypes.cast(out, ctypes.c_void_p), 9)
    assert got == 9, got
    return [int(v) for v in out]


# rows per chunk of the fit, ints per (segment, chunk) record, the chunk count
# above which the ranks are globalized, the gather's positions per pass, the
# new-row limit of tpe_history_order
CHUNK, CNT, PRE_CHUNKS, PASS, NEW = layout(1, 1)[4:9]
MAX_ROWS, MAX_COLS = 3 * PASS + 1, 8


def tkey(v, transform=IDENT, floor=0.0):
    """The fit's key of a value: v, or log(max(v, floor)) (NaN stays NaN)."""
    v = np.array(v, np.float64)
    if transform == LOG:
        with np.errstate(all="ignore"):
            return np.log(np.maximum(v, floor))
    return v


def order_ref(key):
    return np.argsort(key, kind="stable").astype(np.int32)


def dense_ranks(key):
    """Integers ordered as the keys: equal for equal keys (-0.0 and +0.0
    too), every NaN the same and above everything else."""
    o = np.argsort(key, kind="stable")
    s = key[o]
    new = np.ones(s.size, bool)
    new[1:] = ~((s[1:] == s[:-1]) | (np.isnan(s[1:]) & np.isnan(s[:-1])))
    r = np.empty(s.size, np.int64)
    r[o] = np.cumsum(new) - 1
    return r


def merge_step(rank, order_old, n_new):
    """The order of rows [0, n_old + n_new) from the order of [0, n_old), by
    the documented rule."""
    n_old = len(order_old)
    new_rows = n_old + np.argsort(rank[n_old:n_old + n_new], kind="stable")
    old_k, new_k = rank[order_old], rank[new_rows]
    out = np.full(n_old + n_new, -1, np.int32)
    out[np.arange(n_old) + np.searchsorted(new_k, old_k, "left")] = order_old
    dst = np.arange(n_new) + np.searchsorted(old_k, new_k, "right")
    assert (out[dst] == -1).all()
    out[dst] = new_rows
    assert (out >= 0).all()
    return out


def log_separation(v, floor):
    """Smallest relative distance of two different clamped values (inf: none)."""
    u = np.unique(np.maximum(np.asarray(v, np.float64), floor))
    u = u[np.isfinite(u)]
    if u.size < 2:
        return np.inf
    return float(np.min(np.diff(u) / np.abs(u[1:])))


# ---------------------------------------------------------------------------
# stage 1: append
# ---------------------------------------------------------------------------
AppendCase = namedtuple("AppendCase", "name n_labels k r0 ld")
APPEND_SHAPES = ((1, 1), (3, 85), (4, 64), (257, 1), (5, 2049))


def _append_cases():
    out = []
    for nl, k in APPEND_SHAPES:
        for r0 in (0, 11):
            out.append(AppendCase("append-%dx%d-r%d" % (nl, k, r0), nl, k, r0, r0 + k + 5))
    out.append(AppendCase("append-1x1-full", 1, 1, 0, 1))          # r0 + k == ld
    out.append(AppendCase("append-4x64-full", 4, 64, 7, 71))       # r0 + k == ld
    out.append(AppendCase("append-3x85-wide", 3, 85, 100, 100000))  # ld far above the rows
    return out


APPEND = _append_cases()


def append_stage(c):
    """(values (n_labels, k), flags (n_labels, k)) of the case's staged rows."""
    rng = np.random.RandomState(5100 + c.n_labels * 7 + c.k + c.r0)
    return rng.normal(size=(c.n_labels, c.k)), \
        (rng.uniform(size=(c.n_labels, c.k)) < 0.7).astype(np.uint8)


def append_ref(vals, active, sv, sa, r0):
    """The scatter, in place, into vals / active of shape (n_labels, ld)."""
    for l in range(sv.shape[0]):
        for j in range(sv.shape[1]):
            vals[l, r0 + j] = sv[l, j]
            active[l, r0 + j] = sa[l, j]


# ---------------------------------------------------------------------------
# stage 2: order
# ---------------------------------------------------------------------------
OrderCase = namedtuple("OrderCase", "name v transform floor n_old n_new ld")
ORDER_SIZES = ((0, 1), (0, 2), (0, 3), (0, 1023), (0, 1024), (0, 1025), (0, 2047), (0, 2048),
               (1, 1), (255, 2), (256, 3), (257, 1023), (5000, 1024), (1, 1025), (256, 2047),
               (257, 2048), (5000, 2048), (5000, 1), (256, 1), (255, 2048))
ORDER_FULL = ((0, 2048), (257, 1023))   # also with n_old + n_new == ld
ORDER_VALUES = ("random", "equal", "two", "descending", "ascending", "new-below", "new-above",
                "new-in-run", "zeros", "inf", "nan", "log-clamped", "log-nonpositive")
ORDER_SPLITS = ((0, 1500), (1300, 700))


def _order_values(kind, n_old, n_new, rng):
    n = n_old + n_new
    tr, floor = IDENT, 0.0
    if kind == "random":
        v = rng.normal(size=n)
    elif kind == "equal":
        v = np.full(n, 1.5)
    elif kind == "two":
        v = np.where(np.arange(n) % 2 == 0, 1.0, -2.0)
    elif kind == "descending":
        v = (n - np.arange(n)) * 0.25
    elif kind == "ascending":
        v = np.arange(n) * 0.25 - 7.0
    elif kind in ("new-below", "new-above"):
        v = rng.uniform(0.0, 1.0, n)
        v[n_old:] += -2.0 if kind == "new-below" else 2.0
    elif kind == "new-in-run":
        # most old rows tie at 3.0, every new row is 3.0: old before new
        v = np.where(rng.uniform(size=n) < 0.8, 3.0, np.round(rng.normal(3.0, 2.0, n)))
        v[n_old:] = 3.0
    elif kind == "zeros":
        v = rng.choice([-0.0, 0.0, 0.0, -0.0, 1.0, -1.0], n)
    elif kind == "inf":
        v = np.round(rng.normal(size=n), 1)
        v[rng.uniform(size=n) < 0.1] = np.inf
        v[rng.uniform(size=n) < 0.1] = -np.inf
    elif kind == "nan":
        v = np.round(rng.normal(size=n), 1)
        v[rng.uniform(size=n) < 0.15] = np.nan
        v[rng.uniform(size=n) < 0.02] = np.inf
    elif kind == "log-clamped":
        # below exp(0) = 1 for a third of the rows: clamped, tied
        v, tr, floor = np.round(np.exp(rng.uniform(-1.5, 3.0, n)), 2), LOG, 1.0
        assert 0.25 < (v < floor).mean() < 0.4
    elif kind == "log-nonpositive":
        v = rng.choice([0.0, -0.0, -1.0, -300.0, 0.25, 0.5, 0.75, 2.0, 7.0, 1000.0], n)
        tr, floor = LOG, 0.5
    else:
        raise KeyError(kind)
    return np.asarray(v, np.float64), tr, floor


def _order_cases():
    out = []
    for n_old, n_new in ORDER_SIZES:
        rng = np.random.RandomState(5200 + 3 * n_old + n_new)
        v = np.round(rng.normal(size=n_old + n_new), 2)  # (ties at the larger sizes)
        out.append(OrderCase("size-%d+%d" % (n_old, n_new), v, IDENT, 0.0, n_old, n_new,
                             n_old + n_new + 13))
    for n_old, n_new in ORDER_FULL:
        rng = np.random.RandomState(5300 + n_old)
        out.append(OrderCase("full-%d+%d" % (n_old, n_new), np.round(rng.normal(size=n_old + n_new), 2),
                             IDENT, 0.0, n_old, n_new, n_old + n_new))
    for i, kind in enumerate(ORDER_VALUES):
        for n_old, n_new in ORDER_SPLITS:
            rng = np.random.RandomState(5400 + 2 * i + (n_old > 0))
            v, tr, floor = _order_values(kind, n_old, n_new, rng)
            out.append(OrderCase("%s-%d+%d" % (kind, n_old, n_new), v, tr, floor, n_old, n_new,
                                 n_old + n_new + 13))
    for c in out:
        c.v.setflags(write=False)
    return out


ORDER = _order_cases()
ORDER_BY_NAME = {c.name: c for c in ORDER}

# one column of 5000 rows ordered in pieces
PIECES_ROWS = 5000
PIECES = {"three": [2048, 2048, 904],
          "rows-first": [1] * 40 + [1, 7, 2048, 2049 - 1, PIECES_ROWS - 40 - 1 - 7 - 2048 - 2048]}
assert all(sum(p) == PIECES_ROWS and max(p) <= NEW for p in PIECES.values())


def pieces_columns():
    """(values (2, 5000), specs [(col, transform, floor)]): an identity column
    with ties, NaN and infinities, a log column with clamped ties."""
    rng = np.random.RandomState(5500)
    a = np.round(rng.normal(size=PIECES_ROWS), 1)
    a[rng.uniform(size=PIECES_ROWS) < 0.01] = np.nan
    a[rng.uniform(size=PIECES_ROWS) < 0.01] = -np.inf
    b = np.round(np.exp(rng.uniform(-1.5, 3.0, PIECES_ROWS)))
    return np.stack([a, b]), [(0, IDENT, 0.0), (1, LOG, 1.0)]


def multi_spec_case():
    """A four-column history, specs for columns {2, 0} (identity, log), 300 old
    rows and 500 new ones under ld = 1000."""
    rng = np.random.RandomState(5600)
    n_old, n_new, ld = 300, 500, 1000
    vals = rng.normal(size=(4, n_old + n_new))
    vals[2] = np.round(vals[2], 1)
    vals[0] = np.round(np.exp(rng.uniform(-1.5, 3.0, n_old + n_new)))
    return vals, [(2, IDENT, 0.0), (0, LOG, 1.0)], n_old, n_new, ld


# ---------------------------------------------------------------------------
# stage 3: the sorted fit
# ---------------------------------------------------------------------------
# claim: added to the true count in the segment's descriptor (0 but in the
# count-mismatch case)
Seg = namedtuple("Seg", "col below transform floor prior_mu prior_sigma prior_weight lf "
                        "bounded low high claim")
FitCase = namedtuple("FitCase", "name vals active losses n_below segs")
FitReplay = namedtuple("FitReplay", "member cnt local glob n prior_pos mu w_raw w sigma")
FIT_ROWS = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1, 3 * CHUNK + 1)
PMU, PSIG = 0.0, 3.0          # identity columns' prior
LOG_PMU, LOG_PSIG = 1.5, 3.0  # log columns' prior; their floor is 1.0


def seg(col, below, log=False, prior_mu=None, prior_sigma=None, prior_weight=1.0, lf=25,
        bounded=0, claim=0):
    pmu = (LOG_PMU if log else PMU) if prior_mu is None else prior_mu
    ps = (LOG_PSIG if log else PSIG) if prior_sigma is None else prior_sigma
    return Seg(col, int(below), LOG if log else IDENT, 1.0 if log else 0.0, pmu, ps,
               prior_weight, lf, bounded, -6.0, 6.0, claim)


def _fit_case(name, cols, actives, flags, segs):
    """flags: the rows of the below side.  The case keeps losses and n_below,
    from which ap_split_trials forms the same split."""
    flags = np.asarray(flags, bool)
    vals = np.stack([np.asarray(c, np.float64) for c in cols])
    active = np.stack([np.asarray(a, bool) for a in actives]).astype(np.uint8)
    assert vals.shape == active.shape and vals.shape[1] == flags.size
    assert vals.shape[0] <= MAX_COLS and flags.size <= MAX_ROWS
    losses = 1.0 - flags  # (ties: the stable split takes the flagged rows first)
    for a in (vals, active, losses):
        a.setflags(write=False)
    return FitCase(name, vals, active, losses, int(flags.sum()), tuple(segs))


def is_below(c):
    f = np.zeros(c.losses.size, np.uint8)
    f[np.argsort(c.losses, kind="stable")[:c.n_below]] = 1
    return f


def _tied(rng, n):
    return np.round(rng.normal(0.0, 2.0, n), 1)


def _some(rng, n, p=0.5):
    f = rng.uniform(size=n) < p
    return f


def fit_cases(N):
    """The cases at n_rows = N (those that fit into N rows)."""
    rng = np.random.RandomState(6000 + N)
    nch = (N + CHUNK - 1) // CHUNK
    tag = "fit-%d-" % N
    ones, none = np.ones(N, bool), np.zeros(N, bool)
    out = []
    # -- several segments: both sides of an identity column (bounded) and of a
    #    log column with clamped ties, a fifth with no members; 30 % inactive
    flags = none.copy()
    flags[rng.permutation(N)[:min(int(np.ceil(0.25 * np.sqrt(N))), 25)]] = True
    logcol = np.round(np.exp(rng.uniform(-1.5, 3.0, N)))
    out.append(_fit_case(tag + "several", [_tied(rng, N), logcol, _tied(rng, N)],
                         [_some(rng, N, 0.7), _some(rng, N, 0.7), none], flags,
                         [seg(0, 1, bounded=1), seg(0, 0, bounded=1), seg(1, 1, log=True),
                          seg(1, 0, log=True), seg(2, 0)]))
    # -- members in the last chunk only
    last = np.arange(N) >= (nch - 1) * CHUNK
    out.append(_fit_case(tag + "last-chunk", [_tied(rng, N)], [last], _some(rng, N),
                         [seg(0, 1), seg(0, 0)]))
    # -- the only member is the last row: n == 1, the observation below, equal
    #    to and above the prior mean; n == 0 on the other side
    only = none.copy()
    only[N - 1] = True
    cols = [np.where(only, PMU + d, _tied(rng, N)) for d in (-1.0, 0.0, 1.0)]
    out.append(_fit_case(tag + "last-row", cols, [only] * 3, only,
                         [seg(0, 1), seg(1, 1), seg(2, 1), seg(0, 0)]))
    if N >= 2:
        # -- n == 2: the first and the last row
        two = none.copy()
        two[[0, N - 1]] = True
        v = _tied(rng, N)
        v[[0, N - 1]] = [2.0, -1.0]
        out.append(_fit_case(tag + "two", [v], [two], ones, [seg(0, 1), seg(0, 0)]))
        # -- every member below the prior mean, every member above it
        out.append(_fit_case(tag + "one-side", [rng.uniform(-5.0, -1.0, N), rng.uniform(1.0, 5.0, N)],
                             [_some(rng, N, 0.9), _some(rng, N, 0.9)], _some(rng, N),
                             [seg(0, 1), seg(0, 0), seg(1, 1), seg(1, 0)]))
    # -- every row a member; LF = 0; a prior weight other than 1
    out.append(_fit_case(tag + "all", [_tied(rng, N)], [ones], ones,
                         [seg(0, 1), seg(0, 0), seg(0, 1, lf=0), seg(0, 1, prior_weight=0.3),
                          seg(0, 1, prior_weight=7.5, lf=3)]))
    if N >= 5:
        # -- three members equal to the prior mean: the prior goes to their left
        v = _tied(rng, N)
        act = _some(rng, N, 0.8)
        for r in (0, N // 2, N - 1):
            v[r], act[r] = PMU, True
        out.append(_fit_case(tag + "prior-ties", [v], [act], ones, [seg(0, 1)]))
    # -- the sorted order is the reverse of the row order: the ramp lands reversed
    desc = (N - np.arange(N)) * 0.5 - 0.25 * N
    cols, acts = [], []
    for n in (25, 26, 27, 200):
        if n <= N:
            a = none.copy()
            a[np.unique(np.round(np.linspace(0, N - 1, n)).astype(int))] = True
            assert a.sum() == n
            cols.append(desc)
            acts.append(a)
    if cols:
        out.append(_fit_case(tag + "reverse", cols, acts, ones,
                             [seg(j, 1, lf=25) for j in range(len(cols))]))
    # -- members on both sides of every chunk edge, the row at the edge inactive
    if nch > 1:
        a = none.copy()
        for e in range(CHUNK, N, CHUNK):
            a[max(e - 3, 0):min(e + 4, N)] = True
            a[e] = False
        f = np.arange(N) % 2 == 0
        out.append(_fit_case(tag + "edges", [_tied(rng, N)], [a], f, [seg(0, 1, lf=2), seg(0, 0, lf=2)]))
    return out


def mismatch_case(delta):
    """Three segments of one call, the middle one claiming count + delta."""
    N = CHUNK + 1
    rng = np.random.RandomState(6900)
    return _fit_case("fit-mismatch%+d" % delta, [_tied(rng, N), _tied(rng, N)],
                     [_some(rng, N, 0.7), _some(rng, N, 0.7)], _some(rng, N, 0.3),
                     [seg(0, 1), seg(1, 1, claim=delta), seg(1, 0)])


def seg_key(c, s):
    return tkey(c.vals[s.col], s.transform, s.floor)


def seg_lists(c, s):
    """The segment's observation list as the reference forms it
    (oracle.ap_split_trials), transformed."""
    from oracle import tpe_oracle as O
    T = c.losses.size
    act = c.active[s.col] != 0
    gamma = (c.n_below - 0.5) / np.sqrt(T) if c.n_below else 0.0
    below, above = O.ap_split_trials(np.flatnonzero(act), c.vals[s.col][act], np.arange(T),
                                     c.losses, gamma, gamma_cap=T + 1)
    return tkey(below if s.below else above, s.transform, s.floor)


def fit_replay(c, s, order=None):
    """What tpe_fit_sorted leaves for one segment, from the column's order."""
    N = c.losses.size
    nch = max(1, (N + CHUNK - 1) // CHUNK)
    key = seg_key(c, s)
    if order is None:
        order = order_ref(key)
    isb = is_below(c)
    member = [bool(c.active[s.col, r]) and int(isb[r]) == s.below for r in range(N)]
    cnt = np.zeros((nch, CNT), np.int32)
    cnt[:, 2] = INT32_MAX
    local, glob = np.full(N, -1, np.int32), np.full(N, -1, np.int32)
    n = 0
    for r in range(N):           # rows in tid order
        q = r // CHUNK
        if member[r]:
            local[r], glob[r] = cnt[q, 0], n
            cnt[q, 0] += 1
            cnt[q, 1] += 1 if key[r] < s.prior_mu else 0
            cnt[q, 2] = min(cnt[q, 2], r)
            n += 1
    for e in range(N):           # entries in sorted order
        if member[order[e]]:
            cnt[e // CHUNK, 3] += 1
    base = np.cumsum(cnt[:, 0]) - cnt[:, 0]
    if n >= 2:
        prior_pos = int(cnt[:, 1].sum())
    elif n == 1:
        prior_pos = 0 if s.prior_mu < key[int(cnt[:, 2].min())] else 1
    else:
        prior_pos = 0
    if s.lf and s.lf < n:   # the ramp over list positions, the last lf at 1
        ramp = np.concatenate([np.linspace(1.0 / n, 1.0, n - s.lf), np.ones(s.lf)])
    else:
        ramp = np.ones(n)
    mu, w = np.empty(n + 1), np.empty(n + 1)
    p = 0
    for e in range(N):
        row = int(order[e])
        if local[row] >= 0:
            pos = p + (1 if p >= prior_pos else 0)
            mu[pos] = key[row]
            w[pos] = ramp[base[row // CHUNK] + local[row]]
            p += 1
    assert p == n
    mu[prior_pos], w[prior_pos] = s.prior_mu, s.prior_weight
    # the fit's tail: bandwidths, clip, the prior's own sigma, normalisation
    ps = s.prior_sigma
    if n == 0:
        sig = np.array([ps])
    elif n == 1:
        sig = np.full(2, 0.5 * ps)
    else:
        gap = np.diff(mu)
        sig = np.empty(n + 1)
        sig[0], sig[-1] = gap[0], gap[-1]
        sig[1:-1] = np.maximum(gap[:-1], gap[1:])
    sig = np.clip(sig, ps / min(100.0, 1.0 + (n + 1)), ps)
    sig[prior_pos] = ps
    return FitReplay(np.array(member), cnt, local, glob, n, prior_pos, mu, w, w / w.sum(), sig)


# ---------------------------------------------------------------------------
# stage 4: the gathers
# ---------------------------------------------------------------------------
# count: None = the matches; rows: None = identity
Desc = namedtuple("Desc", "col below to_int offset count hist")
GatherCase = namedtuple("GatherCase", "name vals active rows is_below descs")
GATHER_ROWS = (1, 1023, 1024, 1025, PASS - 1, PASS, PASS + 1, 2 * PASS + 1, 3 * PASS + 1)
RANDINT_LOW = 3


def desc(col, below, to_int=0, offset=0, count=None, hist=0):
    return Desc(col, int(below), to_int, offset, count, hist)


def _gather_case(name, vals, active, rows, isb, descs):
    vals, active = np.asarray(vals, np.float64), np.asarray(active, bool).astype(np.uint8)
    isb = np.asarray(isb, bool).astype(np.uint8)
    rows = None if rows is None else np.asarray(rows, np.int32)
    n_pos = isb.size
    assert vals.shape == active.shape and vals.shape[0] <= MAX_COLS and vals.shape[1] <= MAX_ROWS
    assert n_pos <= MAX_ROWS and (rows.size == n_pos if rows is not None else n_pos <= vals.shape[1])
    for a in (vals, active, isb) + (() if rows is None else (rows,)):
        a.setflags(write=False)
    return GatherCase(name, vals, active, rows, isb, tuple(descs))


def _patterns(N, rng):
    """Seven activity patterns of N rows: none, all, only row PASS, only the
    last row, nothing in the first pass and everything after it, alternating,
    random with 30 % inactive."""
    r = np.arange(N)
    at_pass = r == PASS          # (empty below PASS + 1 rows)
    return [np.zeros(N, bool), np.ones(N, bool), at_pass, r == N - 1, r >= PASS, r % 2 == 1,
            rng.uniform(size=N) >= 0.3]


def gather_size_cases(N):
    """Two calls at N rows: every pattern as the below side of a column of its
    own (every flag set, so the members are the active rows; the above side
    of the all-active column has none), and both sides of three patterns under
    random flags."""
    rng = np.random.RandomState(7000 + N)
    pats = _patterns(N, rng)
    vals = rng.normal(size=(len(pats), N))
    a = _gather_case("gather-%d-patterns" % N, vals, pats, None, np.ones(N, bool),
                     [desc(j, 1) for j in range(len(pats))] + [desc(1, 0)])
    b = _gather_case("gather-%d-sides" % N, vals, pats, None, rng.uniform(size=N) < 0.4,
                     [desc(j, side) for j in (1, 5, 6) for side in (1, 0)])
    return [a, b]


def _matches(c, d):
    rows = np.arange(c.is_below.size) if c.rows is None else c.rows
    return int(((c.active[d.col][rows] != 0) & (c.is_below == d.below)).sum())


def _descriptor_cases():
    out = []
    rng = np.random.RandomState(7100)
    N = PASS + 1
    # -- several descriptors: both sides of two fp64 columns, a randint column
    #    as int64 with offsets 0 and 3
    vals = rng.normal(size=(3, N))
    vals[2] = rng.randint(0, 6, N) + RANDINT_LOW
    act = rng.uniform(size=(3, N)) >= 0.3
    isb = rng.uniform(size=N) < 0.4
    out.append(_gather_case("several", vals, act, None, isb,
                            [desc(0, 1), desc(0, 0), desc(1, 1), desc(1, 0),
                             desc(2, 1, to_int=1, offset=0), desc(2, 0, to_int=1, offset=RANDINT_LOW)]))
    # -- a row list: a sorted subset longer than one pass, and a permutation
    ld = 2 * PASS + 100
    vals = rng.normal(size=(2, ld))
    vals[1] = rng.randint(0, 6, ld) + RANDINT_LOW
    act = rng.uniform(size=(2, ld)) >= 0.3
    sub = np.sort(rng.permutation(ld)[:PASS + 500])
    out.append(_gather_case("rows-subset", vals, act, sub, rng.uniform(size=sub.size) < 0.4,
                            [desc(0, 1), desc(0, 0), desc(1, 0, to_int=1, offset=RANDINT_LOW)]))
    perm = rng.permutation(N)
    out.append(_gather_case("rows-permutation", vals[:, :N], act[:, :N], perm,
                            rng.uniform(size=N) < 0.4,
                            [desc(0, 1), desc(0, 0), desc(1, 1, to_int=1, offset=RANDINT_LOW)]))
    # -- a count other than the matches
    N = 2 * PASS + 1
    vals = rng.normal(size=(1, N))
    act = rng.uniform(size=(1, N)) >= 0.1
    base = _gather_case("count", vals, act, None, np.ones(N, bool), [desc(0, 1)])
    m = _matches(base, base.descs[0])
    assert m > PASS + 5
    for name, count in (("count-short-1", m - 1), ("count-short-pass", m - PASS - 5),
                        ("count-long-2", m + 2)):
        out.append(base._replace(name=name, descs=(desc(0, 1, count=count),)))
    return out


GATHER_SPECIAL = _descriptor_cases()
GATHER_SPECIAL_BY_NAME = {c.name: c for c in GATHER_SPECIAL}


def multi_case():
    """Three histories for one tpe_gather_obs_multi launch -- 40 rows (less
    than a wave), PASS + 1 positions through a row list, 2 PASS + 1 identity
    rows -- as single-history cases whose descriptors name their history; and
    the launch's descriptor order, interleaved: (history, index in its case)."""
    rng = np.random.RandomState(7200)
    hs = []
    for h, (n_pos, ld, listed) in enumerate(((40, 50, False), (PASS + 1, PASS + 50, True),
                                             (2 * PASS + 1, 2 * PASS + 1, False))):
        vals = rng.normal(size=(3, ld))
        vals[2] = rng.randint(0, 6, ld) + RANDINT_LOW
        act = rng.uniform(size=(3, ld)) >= 0.3
        rows = rng.permutation(ld)[:n_pos] if listed else None
        ds = [desc(0, 1, hist=h), desc(0, 0, hist=h), desc(1, 0, hist=h),
              desc(2, 1, to_int=1, offset=RANDINT_LOW, hist=h)]
        hs.append(_gather_case("multi-h%d" % h, vals, act, rows, rng.uniform(size=n_pos) < 0.4, ds))
    launch = [(h, i) for i in range(4) for h in (2, 0, 1)]
    return hs, launch


def gather_ref(c, d):
    """Every match of descriptor d, in position order."""
    V, A, isb = c.vals[d.col].tolist(), c.active[d.col].tolist(), c.is_below.tolist()
    rows = None if c.rows is None else c.rows.tolist()
    out = []
    for i in range(len(isb)):
        r = i if rows is None else rows[i]
        if A[r] and isb[i] == d.below:
            out.append(int(V[r]) - d.offset if d.to_int else V[r])
    return np.array(out, np.int64 if d.to_int else np.float64)


@functools.lru_cache(maxsize=None)
def size_cases(kind, N):
    return tuple({"fit": fit_cases, "gather": gather_size_cases}[kind](N))
