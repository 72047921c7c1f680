"""The history cases (tests/history_cases.py) are what they are named for, and
the numpy restatements of the stages agree with the oracle -- without a GPU.

  * tpe_fit_sorted_layout is host code: its nine numbers, and that the sizes
    the case tables are cut by come from it;
  * the order reference built in pieces by the documented merge rule equals
    the single stable argsort; every log column keeps the 1e-9 separation;
  * the stage-3 replay -- chunk counts, rank words, the mixture assembled from
    them -- ends in oracle.adaptive_parzen_normal's (w, mu, sigma) and prior
    slot on the lists oracle.ap_split_trials gives, on every case;
  * three slips restated on the replay (the first member taken from chunk 0,
    the ramp by sorted position, a gather without its carry or its count
    guard) change what the GPU tests compare;
  * every case is small.
tests/test_gpu_history_stages.py runs the kernels on the same tables.
"""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _lib as L
from oracle import tpe_oracle as O
from tests import history_cases as HC


# -- the layout entry ---------------------------------------------------------------
def _layout(lib, n_seg, n_rows, n=9):
    out = (ctypes.c_int64 * 10)(*([-7] * 10))
    rc = lib.tpe_fit_sorted_layout(n_seg, n_rows, ctypes.cast(out, ctypes.c_void_p), n)
    return rc, list(out)


def test_layout_is_consistent():
    lib = L.load()
    chunk = None
    for n_seg in (0, 1, 2, 5, 64):
        for n_rows in (0, 1, 1023, 1024, 1025, 3073, 5000, 2 ** 22, 2 ** 22 + 1, 2 ** 31 - 1):
            rc, out = _layout(lib, n_seg, n_rows)
            assert rc == 9 and out[9] == -7, (n_seg, n_rows)
            gi, cnt, part, total, chunk, ints, pre, gpass, new = out[:9]
            chunks = max(1, (n_rows + chunk - 1) // chunk)
            segs = max(n_seg, 1)
            assert gi == 0 and cnt - gi >= 4 * segs * n_rows
            assert part - cnt >= 4 * ints * segs * chunks and total >= part
            assert cnt % 8 == 0 and part % 8 == 0
            assert total == lib.tpe_fit_sorted_scratch_bytes(n_seg, n_rows)
    assert (chunk, ints, pre, gpass, new) == (HC.CHUNK, HC.CNT, HC.PRE_CHUNKS, HC.PASS, HC.NEW)
    assert ints == 4 and chunk > 0 and gpass % chunk == 0 and new > 0 and pre > 0
    # fewer entries than nine: that many are written
    rc, out = _layout(lib, 3, 5000, 4)
    assert rc == 4 and out[4:] == [-7] * 6 and out[:4] == _layout(lib, 3, 5000)[1][:4]
    assert lib.tpe_fit_sorted_layout(3, 5000, None, 0) == 0


def test_layout_argument_errors():
    lib = L.load()
    for n_seg, n_rows, n in ((-1, 1, 9), (1, -1, 9), (1, 1, -1), (1, 2 ** 31, 9)):
        assert _layout(lib, n_seg, n_rows, n)[0] == -1, (n_seg, n_rows, n)
        assert b"tpe_fit_sorted_layout" in lib.tpe_last_error()
    assert lib.tpe_fit_sorted_layout(1, 1, None, 9) == -1


def test_the_tables_sit_on_the_reported_edges():
    C, P = HC.CHUNK, HC.PASS
    assert HC.FIT_ROWS == (1, 2, C - 1, C, C + 1, 2 * C, 2 * C + 1, 3 * C + 1)
    assert HC.GATHER_ROWS == (1, 1023, 1024, 1025, P - 1, P, P + 1, 2 * P + 1, 3 * P + 1)
    new = {c.n_new for c in HC.ORDER}
    assert new >= {1, 2, 3, 1023, 1024, 1025, HC.NEW - 1, HC.NEW}
    for k in (1, 2, 3, 1023, 1024, 1025, HC.NEW - 1, HC.NEW):
        olds = {c.n_old for c in HC.ORDER if c.n_new == k}
        assert 0 in olds and max(olds) > 0, k
    assert {c.n_old for c in HC.ORDER} >= {0, 1, 255, 256, 257, 5000}
    assert any(c.n_old + c.n_new == c.ld for c in HC.ORDER)
    for kind in HC.ORDER_VALUES:
        assert sum(c.name.startswith(kind + "-") for c in HC.ORDER) == 2
    shapes = {(c.n_labels, c.k) for c in HC.APPEND}
    assert shapes == set(HC.APPEND_SHAPES) and {3 * 85, 4 * 64} == {255, 256}
    assert {c.r0 == 0 for c in HC.APPEND} == {True, False}
    assert any(c.r0 + c.k == c.ld for c in HC.APPEND)
    assert any(c.ld > 100 * (c.r0 + c.k) for c in HC.APPEND)


def test_every_case_is_small():
    rows = cols = 0
    for c in HC.ORDER:
        rows = max(rows, c.v.size)
    for N in HC.FIT_ROWS:
        for c in HC.fit_cases(N):
            rows, cols = max(rows, c.vals.shape[1]), max(cols, c.vals.shape[0])
    for N in HC.GATHER_ROWS:
        for c in HC.gather_size_cases(N):
            rows, cols = max(rows, c.vals.shape[1]), max(cols, c.vals.shape[0])
    for c in list(HC.GATHER_SPECIAL) + HC.multi_case()[0]:
        rows, cols = max(rows, c.vals.shape[1]), max(cols, c.vals.shape[0])
    assert rows == HC.MAX_ROWS == 3 * HC.PASS + 1 == 49153 and cols <= HC.MAX_COLS == 8
    assert HC.PIECES_ROWS <= HC.MAX_ROWS


# -- stage 1 -----------------------------------------------------------------------
def test_append_reference():
    c = HC.APPEND[2]
    sv, sa = HC.append_stage(c)
    vals, act = np.full((c.n_labels, c.ld), -9.0), np.full((c.n_labels, c.ld), 77, np.uint8)
    HC.append_ref(vals, act, sv, sa, c.r0)
    np.testing.assert_array_equal(vals[:, c.r0:c.r0 + c.k], sv)
    np.testing.assert_array_equal(act[:, c.r0:c.r0 + c.k], sa)
    assert (vals[:, :c.r0] == -9.0).all() and (vals[:, c.r0 + c.k:] == -9.0).all()
    assert (act[:, :c.r0] == 77).all() and (act[:, c.r0 + c.k:] == 77).all()
    assert set(np.unique(sa).tolist()) == {0, 1}


# -- stage 2 -----------------------------------------------------------------------
def test_keys_and_ranks():
    v = np.array([np.nan, 3.0, -0.0, np.inf, 0.0, -np.inf, -np.nan, 3.0, -1.0])
    r = HC.dense_ranks(v)
    assert r[0] == r[6] == r.max() and r[2] == r[4] and r[1] == r[7]
    assert r[5] < r[8] < r[2] < r[1] < r[3] < r[0]
    np.testing.assert_array_equal(HC.order_ref(v), [5, 8, 2, 4, 1, 7, 3, 0, 6])
    k = HC.tkey([0.0, -2.0, 0.5, 0.25, 4.0, np.nan, np.inf], HC.LOG, 0.5)
    np.testing.assert_array_equal(k[:4], np.log(0.5))
    assert k[4] == np.log(4.0) and np.isnan(k[5]) and k[6] == np.inf


@pytest.mark.parametrize("c", HC.ORDER, ids=lambda c: c.name)
def test_merge_rule_is_the_stable_argsort(c):
    n = c.n_old + c.n_new
    assert c.v.size == n <= c.ld and 0 < c.n_new <= HC.NEW
    key = HC.tkey(c.v, c.transform, c.floor)
    want = HC.order_ref(key)
    rank = HC.dense_ranks(key)
    got = HC.merge_step(rank, HC.order_ref(key[:c.n_old]), c.n_new)
    np.testing.assert_array_equal(got, want)
    if c.transform == HC.LOG:
        assert HC.log_separation(c.v, c.floor) >= 1e-9
        finite = key[np.isfinite(key)]
        assert np.abs(finite).max() < 10.0
    # what the case is named for
    kind = c.name.rsplit("-", 1)[0]
    old, new = np.arange(n) < c.n_old, np.arange(n) >= c.n_old
    if kind == "equal":
        np.testing.assert_array_equal(want, np.arange(n))
    elif kind == "two":
        np.testing.assert_array_equal(want, np.concatenate([np.arange(1, n, 2), np.arange(0, n, 2)]))
    elif kind == "descending":
        np.testing.assert_array_equal(want, np.arange(n)[::-1])
    elif kind == "ascending":
        np.testing.assert_array_equal(want, np.arange(n))
    elif kind == "new-below" and c.n_old:
        assert new[want[:c.n_new]].all()
    elif kind == "new-above" and c.n_old:
        assert old[want[:c.n_old]].all()
    elif kind == "new-in-run":
        run = want[c.v[want] == 3.0]
        assert run.size >= c.n_new + 0.5 * c.n_old and (np.diff(run) > 0).all()
    elif kind == "zeros":
        z = want[c.v[want] == 0.0]
        assert np.signbit(c.v[z]).any() and not np.signbit(c.v[z]).all() and (np.diff(z) > 0).all()
        assert (np.diff(np.signbit(c.v[z]).astype(int)) != 0).sum() > 10  # (signs interleaved)
    elif kind == "inf":
        assert c.v[want[0]] == -np.inf and c.v[want[-1]] == np.inf
        assert np.isinf(c.v[new]).any() and (not c.n_old or np.isinf(c.v[old]).any())
    elif kind == "nan":
        k = int(np.isnan(c.v).sum())
        assert k > 10 and np.isnan(c.v[want[-k:]]).all() and (np.diff(want[-k:]) > 0).all()
        assert c.v[want[-k - 1]] == np.inf
    elif kind == "log-clamped":
        k = int((c.v <= c.floor).sum())
        assert k > n / 5 and (np.diff(want[:k]) > 0).all() and (c.v[want[:k]] <= c.floor).all()
    elif kind == "log-nonpositive":
        k = int((c.v <= c.floor).sum())
        assert (c.v <= 0).sum() > n / 5 and (np.diff(want[:k]) > 0).all()


@pytest.mark.parametrize("schedule", sorted(HC.PIECES))
def test_order_in_pieces_is_the_stable_argsort(schedule):
    vals, specs = HC.pieces_columns()
    for col, tr, floor in specs:
        key = HC.tkey(vals[col], tr, floor)
        rank = HC.dense_ranks(key)
        if tr == HC.LOG:
            assert HC.log_separation(vals[col], floor) >= 1e-9
        order = np.zeros(0, np.int32)
        for k in HC.PIECES[schedule]:
            order = HC.merge_step(rank, order, k)
            np.testing.assert_array_equal(order, HC.order_ref(key[:order.size]))
        assert order.size == HC.PIECES_ROWS
    assert HC.PIECES["rows-first"][:41] == [1] * 41
    vals, specs, n_old, n_new, ld = HC.multi_spec_case()
    assert [s[0] for s in specs] == [2, 0] and vals.shape == (4, n_old + n_new) and n_old + n_new < ld
    assert HC.log_separation(vals[0], 1.0) >= 1e-9


# -- stage 3 -----------------------------------------------------------------------
def _plain_list(c, s):
    isb = HC.is_below(c)
    key = HC.seg_key(c, s)
    return np.array([key[r] for r in range(isb.size)
                     if c.active[s.col, r] and isb[r] == s.below], np.float64)


def _check_replay(c, s):
    obs = HC.seg_lists(c, s)
    np.testing.assert_array_equal(obs, _plain_list(c, s), err_msg=c.name)
    r = HC.fit_replay(c, s)
    ow, omu, osig = O.adaptive_parzen_normal(obs, s.prior_weight, s.prior_mu, s.prior_sigma, s.lf)
    assert r.n == obs.size and r.mu.size == obs.size + 1
    np.testing.assert_array_equal(r.mu, omu, err_msg=c.name)
    np.testing.assert_array_equal(r.sigma, osig, err_msg=c.name)
    np.testing.assert_array_equal(r.w, ow, err_msg=c.name)
    # the prior's slot: the only component with the prior's sigma and raw weight
    # where that is decidable, else searchsorted 'left' / the len == 1 rule
    if r.n >= 2:
        assert r.prior_pos == int(np.searchsorted(np.sort(obs, kind="stable"), s.prior_mu))
    elif r.n == 1:
        assert r.prior_pos == (0 if s.prior_mu < obs[0] else 1)
    assert r.mu[r.prior_pos] == s.prior_mu and r.sigma[r.prior_pos] == s.prior_sigma
    # the words and counts among themselves
    base = np.cumsum(r.cnt[:, 0]) - r.cnt[:, 0]
    m = r.member
    np.testing.assert_array_equal(r.glob[m], base[np.flatnonzero(m) // HC.CHUNK] + r.local[m])
    np.testing.assert_array_equal(r.glob[m], np.arange(r.n))
    assert (r.local[~m] == -1).all() and r.cnt[:, 0].sum() == r.cnt[:, 3].sum() == r.n
    if s.transform == HC.LOG:
        assert HC.log_separation(c.vals[s.col], s.floor) >= 1e-9
        assert np.abs(HC.seg_key(c, s)).max() < 10.0
    return r


@pytest.mark.parametrize("N", HC.FIT_ROWS)
def test_fit_replay_is_the_oracle(N):
    C = HC.CHUNK
    cases = {c.name.split("-", 2)[2]: c for c in HC.size_cases("fit", N)}
    want = {"several", "last-chunk", "last-row", "all"}
    want |= {"two", "one-side"} if N >= 2 else set()
    want |= {"prior-ties"} if N >= 5 else set()
    want |= {"reverse"} if N >= 25 else set()
    want |= {"edges"} if N > C else set()
    assert set(cases) == want
    nch = (N + C - 1) // C
    R = {name: [_check_replay(c, s) for s in c.segs] for name, c in cases.items()}
    # -- what each case is named for
    r = R["several"]
    assert r[4].n == 0 and r[4].prior_pos == 0 and (r[4].cnt[:, 2] == HC.INT32_MAX).all()
    if N >= C - 1:
        assert min(x.n for x in r[:4]) >= 2
        assert (np.diff(r[2].mu) == 0).sum() > 0 and (r[3].mu == 0.0).sum() > N // 8  # clamped ties
    for x in R["last-chunk"]:
        assert (x.cnt[:-1, 0] == 0).all() and x.cnt[-1, 0] == x.n
    assert sum(x.n for x in R["last-chunk"]) == N - (nch - 1) * C
    a, b, c3, empty = R["last-row"]
    assert [x.n for x in (a, b, c3, empty)] == [1, 1, 1, 0]
    assert [x.prior_pos for x in (a, b, c3)] == [1, 1, 0]
    for x in (a, b, c3):
        assert (x.cnt[:, 2] == [HC.INT32_MAX] * (nch - 1) + [N - 1]).all()
    if N >= 2:
        assert [x.n for x in R["two"]] == [2, 0]
        lo, _, hi, _ = R["one-side"]
        assert lo.prior_pos == lo.n >= (N > 2) and hi.prior_pos == 0 and hi.n >= (N > 2)
    full = R["all"]
    assert full[0].n == N and full[1].n == 0
    if N > 25:
        assert len(np.unique(full[0].w)) > 2 and len(np.unique(full[2].w)) == 1  # ramp, LF = 0
        assert len(np.unique(full[4].w)) > N // 2
    if N >= 5:
        x, = R["prior-ties"]
        s = cases["prior-ties"].segs[0]
        assert (x.mu == s.prior_mu).sum() >= 4 and x.mu[x.prior_pos + 1] == s.prior_mu
        assert x.prior_pos == 0 or x.mu[x.prior_pos - 1] < s.prior_mu
        assert x.w_raw[x.prior_pos] == 1.0
    if N >= 25:
        ns = [x.n for x in R["reverse"]]
        assert ns == [n for n in (25, 26, 27, 200) if n <= N]
        for x in R["reverse"]:
            # ramp entries: none, one, two, many; reversed in the sorted list
            obs_w = np.delete(x.w_raw, x.prior_pos)
            assert (obs_w < 1.0).sum() == max(x.n - 25 - 1, 0) + (x.n == 26)
            assert (np.diff(obs_w) <= 0).all()
            if x.n > 25:
                assert obs_w[-1] == 1.0 / x.n
    if N > C:
        for x in R["edges"]:
            assert (x.cnt[:-1, 0] > 0).all() and 1 <= x.n <= 3 * (nch - 1) + 3
        lo, hi = R["edges"]
        for e in range(C, N, C):   # each neighbour of the edge row is in one of the two lists
            assert lo.local[e] == hi.local[e] == -1
            assert (lo.local[e - 1] >= 0) != (hi.local[e - 1] >= 0)
            assert e + 1 >= N or (lo.local[e + 1] >= 0) != (hi.local[e + 1] >= 0)


def test_mismatch_cases():
    for delta in (-1, 1):
        c = HC.mismatch_case(delta)
        assert [s.claim for s in c.segs] == [0, delta, 0]
        for s in c.segs:
            assert _check_replay(c, s).n > 100


# -- seeded slips, restated on the replay ----------------------------------------
def test_first_from_chunk_zero_would_show():
    """Taking `first` from chunk 0 only leaves INT32_MAX (no member there)
    wherever the only member lies in a later chunk: the last-row cases at more
    than one chunk."""
    for N in HC.FIT_ROWS:
        if N <= HC.CHUNK:
            continue
        c = [x for x in HC.size_cases("fit", N) if x.name.endswith("last-row")][0]
        for s in c.segs[:3]:
            r = HC.fit_replay(c, s)
            assert r.n == 1 and r.cnt[0, 2] == HC.INT32_MAX != r.cnt[:, 2].min() == N - 1


def test_ramp_by_sorted_position_would_show():
    """lf_weight by the sorted position instead of the list position: other
    weights wherever the sorted order is not the row order and a ramp exists."""
    hit = 0
    for N in HC.FIT_ROWS:
        for c in HC.size_cases("fit", N):
            for s in c.segs:
                r = HC.fit_replay(c, s)
                if not (s.lf and s.lf < r.n):
                    continue
                ramp = np.concatenate([np.linspace(1.0 / r.n, 1.0, r.n - s.lf), np.ones(s.lf)])
                wrong = np.insert(ramp, r.prior_pos, s.prior_weight)
                if c.name.endswith("reverse"):
                    assert not np.array_equal(wrong, r.w_raw), c.name
                hit += not np.array_equal(wrong, r.w_raw)
    assert hit > 30


def _gather_slip(c, d, carry=True, guard=True):
    """gather_one pass by pass on the host: (window of `size` slots starting
    from -7, found).  Without the carry every pass starts at slot 0; without
    the guard it writes past `count`."""
    want = HC.gather_ref(c, d)
    count = want.size if d.count is None else d.count
    win = np.full(max(want.size, count) + 4, -7.0)
    rows = np.arange(c.is_below.size) if c.rows is None else c.rows
    take = (c.active[d.col][rows] != 0) & (c.is_below == d.below)
    v = c.vals[d.col][rows]
    done = 0
    for p0 in range(0, take.size, HC.PASS):
        t = take[p0:p0 + HC.PASS]
        pos = (done if carry else 0) + np.cumsum(t) - t
        ok = t & ((pos < count) if guard else True)
        win[pos[ok]] = v[p0:p0 + HC.PASS][ok]
        done += int(t.sum())
    return win, done


def test_gather_slips_would_show():
    """The pass-by-pass restatement equals the reference; without the carry
    every case with members beyond the first pass differs, without the count
    guard the short-count cases write beyond `count`."""
    hit = 0
    for N in HC.GATHER_ROWS:
        for c in HC.size_cases("gather", N):
            for d in c.descs:
                want = HC.gather_ref(c, d)
                win, found = _gather_slip(c, d)
                assert found == want.size and (win[want.size:] == -7).all()
                np.testing.assert_array_equal(win[:want.size], want)
                # (a pass with members after a pass with members)
                t = (c.active[d.col] != 0) & (c.is_below == d.below)
                per = [int(t[p:p + HC.PASS].sum()) for p in range(0, N, HC.PASS)]
                shows = any(per[p] and sum(per[:p]) for p in range(1, len(per)))
                bad, _ = _gather_slip(c, d, carry=False)
                assert shows == (not np.array_equal(bad, win)), c.name
                hit += shows
    assert hit >= 20
    for name in ("count-short-1", "count-short-pass"):
        c = HC.GATHER_SPECIAL_BY_NAME[name]
        d, = c.descs
        win, found = _gather_slip(c, d)
        assert found > d.count and (win[d.count:] == -7).all() and (win[:d.count] != -7).all()
        bad, _ = _gather_slip(c, d, guard=False)
        assert bad[d.count] != -7


# -- stage 4 -----------------------------------------------------------------------
def _mask_list(c, d):
    rows = np.arange(c.is_below.size) if c.rows is None else c.rows
    take = (c.active[d.col][rows] != 0) & (c.is_below == d.below)
    v = c.vals[d.col][rows][take]
    return v.astype(np.int64) - d.offset if d.to_int else v


@pytest.mark.parametrize("N", HC.GATHER_ROWS)
def test_gather_size_cases(N):
    P = HC.PASS
    a, b = HC.size_cases("gather", N)
    for c in (a, b):
        assert c.vals.shape == (7, N) and c.rows is None
        for d in c.descs:
            np.testing.assert_array_equal(HC.gather_ref(c, d), _mask_list(c, d))
    n = [HC.gather_ref(a, d).size for d in a.descs]
    assert n[0] == 0 and n[1] == N and n[2] == (N > P) and n[3] == 1 and n[4] == max(N - P, 0)
    assert n[5] == N // 2 and n[7] == 0 and (N < 100 or 0.6 * N < n[6] < 0.8 * N)
    if N > P:
        assert HC.gather_ref(a, a.descs[2])[0] == a.vals[2, P]
        assert not a.active[4, :P].any() and a.active[4, P:].all()
    assert HC.gather_ref(a, a.descs[3])[0] == a.vals[3, N - 1]
    sides = [HC.gather_ref(b, d).size for d in b.descs]
    assert sides[0] + sides[1] == N and (N < 100 or min(sides) > 0)


def test_gather_descriptor_cases():
    P = HC.PASS
    by = HC.GATHER_SPECIAL_BY_NAME
    for c in HC.GATHER_SPECIAL:
        for d in c.descs:
            got = HC.gather_ref(c, d)
            np.testing.assert_array_equal(got, _mask_list(c, d))
            assert got.dtype == (np.int64 if d.to_int else np.float64)
    c = by["several"]
    assert [(d.to_int, d.offset) for d in c.descs[4:]] == [(1, 0), (1, 3)]
    assert set(HC.gather_ref(c, c.descs[5]).tolist()) == set(range(6))
    assert set(HC.gather_ref(c, c.descs[4]).tolist()) == set(range(3, 9))
    c = by["rows-subset"]
    assert c.rows.size > P and (np.diff(c.rows) > 0).all() and c.rows.size < c.vals.shape[1]
    c = by["rows-permutation"]
    assert sorted(c.rows.tolist()) == list(range(P + 1)) and (np.diff(c.rows) < 0).any()
    m = HC.gather_ref(by["count-short-1"], by["count-short-1"].descs[0]._replace(count=None)).size
    assert [by[n].descs[0].count - m for n in ("count-short-1", "count-short-pass",
                                               "count-long-2")] == [-1, -P - 5, 2]
    hs, launch = HC.multi_case()
    assert [h.is_below.size for h in hs] == [40, P + 1, 2 * P + 1] and 40 < 64
    assert [h.rows is not None for h in hs] == [False, True, False]
    assert len({h.vals.shape[1] for h in hs}) == 3 and len(launch) == 12
    assert [h for h, _ in launch[:3]] == [2, 0, 1]
    for h, i in launch:
        d = hs[h].descs[i]
        assert d.hist == h
        np.testing.assert_array_equal(HC.gather_ref(hs[h], d), _mask_list(hs[h], d))
