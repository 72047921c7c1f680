"""Distinct configurations of a pool: tpe_pool_distinct alone (csrc/
tpe_distinct.hip), tpe.distinct_rows, and distinct=True of suggest_sampled /
suggest_from_pool.

Reference (``reference_first``): a dict from (activity bytes, canonical bytes
of the live values) to the first row that holds the key, the seen rows entered
first as -1 - t.  Everything is compared exactly.
"""
import ctypes
from functools import partial

import numpy as np
import pytest

from hyperopt_amd import (JOB_STATE_DONE, STATUS_FAIL, STATUS_OK, Domain, Trials, fmin, hp, rand,
                          tpe)
from hyperopt_amd import _lib as L
from hyperopt_amd.base import trials_from_docs
from hyperopt_amd.pool import startup_rows
from tests import cond_util as C
from tests.golden import spaces
from tests.test_gpu_pool import _expected_order

pytestmark = pytest.mark.gpu


# -- the reference ----------------------------------------------------------------
def _canonical(v):
    """fp64 values with one zero and one NaN."""
    v = np.array(v, np.float64)
    v[v == 0] = 0.0
    v[np.isnan(v)] = np.nan
    return v


def _key(vals, active):
    active = np.asarray(active, bool)
    return active.tobytes(), _canonical(np.asarray(vals, np.float64)[active]).tobytes()


def reference_first(vals, active, seen_vals=None, seen_active=None):
    """``first`` of the rows of ``vals`` / ``active`` ((n, L), row-major)
    against the seen rows ((T, L), in list order)."""
    table = {}
    if seen_vals is not None:
        for t in range(len(seen_vals)):
            table.setdefault(_key(seen_vals[t], seen_active[t]), -1 - t)
    first = np.empty(len(vals), np.int64)
    for r in range(len(vals)):
        first[r] = table.setdefault(_key(vals[r], active[r]), r)
    return first


# -- 1. the entry point alone -------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _columns(vals, active, ld, rng):
    """(n, L) rows as label-major columns of leading dimension ``ld``; the
    padding holds noise and live flags."""
    n, nl = vals.shape
    cv = rng.normal(size=(nl, ld))
    ca = np.ones((nl, ld), np.uint8)
    cv[:, :n] = vals.T
    ca[:, :n] = active.T
    return cv, ca


def _distinct(cv, ca, n, seen=None, hash_bits=64, taken=None):
    """tpe_pool_distinct through the C ABI: (first, mask), each of the pool's
    leading dimension, poisoned with -7 / 7 beforehand.  ``seen``: (columns,
    activity, ld, row list or None, T, shift or None)."""
    import torch
    lib = L.load()
    nl, ld = cv.shape
    d_v, d_a = _up(cv), _up(ca)
    d_first = torch.full((ld,), -7, dtype=torch.int64, device=_dev())
    d_mask = torch.full((ld,), 7, dtype=torch.uint8, device=_dev())
    sv = sa = rows = shift = None
    sld = T = 0
    keep = []
    if seen is not None:
        scv, sca, sld, srows, T, sshift = seen
        keep = [_up(scv), _up(sca)]
        sv, sa = keep[0].data_ptr(), keep[1].data_ptr()
        if srows is not None:
            keep.append(_up(np.asarray(srows, np.int32)))
            rows = keep[-1].data_ptr()
        if sshift is not None:
            shift = np.ascontiguousarray(sshift, np.float64)
    d_taken = None if taken is None else _up(np.asarray(taken, np.uint8))
    need = lib.tpe_pool_distinct_scratch_bytes(n, T)
    assert need > 0
    d_ws = torch.empty(need, dtype=torch.uint8, device=_dev())
    sp = ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    L.check(lib.tpe_pool_distinct(d_v.data_ptr(), d_a.data_ptr(), ld, n, nl, sv, sa, sld, rows, T,
                                  None if shift is None else shift.ctypes.data, hash_bits,
                                  None if d_taken is None else d_taken.data_ptr(),
                                  d_first.data_ptr(), d_mask.data_ptr(), d_ws.data_ptr(), sp),
            "tpe_pool_distinct")
    return d_first.cpu().numpy(), d_mask.cpu().numpy()


VALUES = np.array([0.0, 1.0, 2.0, -3.5, np.nan, 7.0])
SHIFT = 5.0  # of column 0 of the seen rows


def _base_rows(k, nl, rng):
    """k configurations over a small value set; every fourth one is its
    neighbour with one activity bit flipped (equal values, another label set)."""
    vals = VALUES[rng.randint(0, VALUES.size, (k, nl))]
    active = rng.rand(k, nl) < 0.7
    for i in range(1, k, 4):
        vals[i], active[i] = vals[i - 1], active[i - 1]
        active[i, rng.randint(nl)] ^= True
    return vals, active


def _dress(vals, active, rng):
    """The same configurations in other bytes: zeros of either sign, noise
    where a label is not live."""
    v = vals.copy()
    v[(v == 0) & (rng.rand(*v.shape) < 0.5)] = -0.0
    dead = ~active
    v[dead] = rng.normal(size=int(dead.sum())) * 100
    return v


def _check(first, mask, want, taken, n):
    np.testing.assert_array_equal(first[:n], want)
    assert (first[n:] == -7).all() and (mask[n:] == 7).all()  # the padding is untouched
    t = np.zeros(n, np.uint8) if taken is None else taken
    np.testing.assert_array_equal(mask[:n], t | (want != np.arange(n)))


@pytest.mark.parametrize("nl", [1, 5, 70])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_pool_distinct(n, nl):
    rng = np.random.RandomState(1000 * nl + n)
    k_pool = min(n, 150)
    bv, ba = _base_rows(k_pool + 60, nl, rng)  # at most 210 classes: hash_bits = 0 stays cheap
    pick = rng.randint(0, k_pool, n)
    pv, pa = _dress(bv[pick], ba[pick], rng), ba[pick]
    ld = n + 37
    cv, ca = _columns(pv, pa, ld, rng)
    taken = (rng.rand(n) < 0.3).astype(np.uint8)
    for T in (0, 1, 65, 300):
        # seen rows: some equal pool rows, some equal nothing
        spick = rng.randint(k_pool // 2, k_pool + 60, T)
        sv, sa = _dress(bv[spick], ba[spick], rng), ba[spick]
        stored = sv.copy()
        stored[:, 0] += SHIFT
        shift = np.zeros(nl)
        shift[0] = SHIFT
        want = reference_first(pv, pa, sv, sa) if T else reference_first(pv, pa)
        layouts = [None]
        if T:
            scv, sca = _columns(stored, sa, T + 11, rng)
            layouts = [(scv, sca, T + 11, None, T, shift)]
            # a permuted subset of a larger store; the rows outside the list
            # hold pool row 0 and must not be seen
            m = T + 20
            rows = rng.permutation(m)[:T]
            big_v = np.tile(pv[0] + shift, (m, 1))
            big_a = np.tile(pa[0], (m, 1))
            big_v[rows], big_a[rows] = stored, sa
            bcv, bca = _columns(big_v, big_a, m + 3, rng)
            layouts.append((bcv, bca, m + 3, rows, T, shift))
        for seen in layouts:
            for hash_bits in (64, 4, 0):
                for tk in (None, taken):
                    first, mask = _distinct(cv, ca, n, seen, hash_bits, tk)
                    _check(first, mask, want, tk, n)
                    again = _distinct(cv, ca, n, seen, hash_bits, tk)
                    assert first.tobytes() == again[0].tobytes()
                    assert mask.tobytes() == again[1].tobytes()
    # permuted pool rows: the classes are the same sets of rows, each class's
    # smallest member its first (no seen rows)
    first, _ = _distinct(cv, ca, n)
    perm = rng.permutation(n)
    cv2, ca2 = _columns(pv[perm], pa[perm], ld, rng)
    first2, mask2 = _distinct(cv2, ca2, n)
    _check(first2, mask2, reference_first(pv[perm], pa[perm]), None, n)
    cls = first[perm]  # the class of permuted row i, by its old name
    for c in np.unique(cls):
        members = np.flatnonzero(cls == c)
        assert (first2[members] == members.min()).all()


@pytest.mark.parametrize("hash_bits", [64, 4])
def test_pool_distinct_all_distinct(hash_bits):
    """4097 continuous rows, every row its own class; 16 chains of about 256
    classes with 4 hash bits."""
    rng = np.random.RandomState(7)
    n, nl = 4097, 5
    pv = rng.normal(size=(n, nl))
    pa = np.ones((n, nl), bool)
    cv, ca = _columns(pv, pa, n + 37, rng)
    sv = np.concatenate([pv[[4000, 17]], rng.normal(size=(63, nl))])
    scv, sca = _columns(sv, np.ones(sv.shape, bool), 80, rng)
    first, mask = _distinct(cv, ca, n, (scv, sca, 80, None, 65, None), hash_bits)
    want = np.arange(n)
    want[4000], want[17] = -1, -2
    _check(first, mask, want, None, n)


# -- 2. tpe.distinct_rows -------------------------------------------------------------
def _doc(tid, cfg, labels, loss):
    result = {"status": STATUS_OK, "loss": float(loss)} if loss is not None else \
        {"status": STATUS_FAIL}
    return {"state": JOB_STATE_DONE, "tid": tid, "spec": None, "result": result,
            "misc": {"tid": tid, "cmd": None, "workdir": None,
                     "idxs": {lab: [tid] if lab in cfg else [] for lab in labels},
                     "vals": {lab: [cfg[lab]] if lab in cfg else [] for lab in labels}},
            "exp_key": None, "owner": None, "version": 0, "book_time": None,
            "refresh_time": None}


def _trials_of(domain, configs, losses):
    labels = list(domain.params)
    return trials_from_docs([_doc(t, c, labels, l)
                             for t, (c, l) in enumerate(zip(configs, losses))])


def _doc_config(doc):
    return {k: v[0] for k, v in doc["misc"]["vals"].items() if v}


def _ckey(cfg):
    return tuple(sorted((k, float(v)) for k, v in cfg.items()))


def config_first(pool_configs, seen_configs=()):
    """``first`` from {label: value} dicts."""
    table = {}
    for t, c in enumerate(seen_configs):
        table.setdefault(_ckey(c), -1 - t)
    return np.asarray([table.setdefault(_ckey(c), r) for r, c in enumerate(pool_configs)],
                      np.int64)


def _space(name):
    maker = spaces.SPACES.get(name) or C.CRAFTED[name]
    return Domain(lambda x: 0, maker(hp))


def _arrays(domain, configs):
    labels = list(domain.params)
    vals = np.full((len(configs), len(labels)), -123.0)  # inactive entries are ignored
    active = np.zeros(vals.shape, bool)
    for r, c in enumerate(configs):
        for lab, v in c.items():
            vals[r, labels.index(lab)] = v
            active[r, labels.index(lab)] = True
    return vals, active


@pytest.mark.parametrize("device_history", [True, False])
@pytest.mark.parametrize("space", ["nested", "shared_node", "pchoice_nested"])
def test_distinct_rows(space, device_history, monkeypatch):
    monkeypatch.setattr(tpe, "USE_DEVICE_HISTORY", device_history)
    domain = _space(space)
    rng = np.random.RandomState(11)
    base = [rand.sample_config(domain, rng) for _ in range(60)]
    rows = [base[i] for i in rng.randint(0, 40, 300)]          # 300 rows over <= 40 classes
    seen = [base[i] for i in rng.randint(30, 60, 45)]          # some of them, and others
    pool = tpe.Pool.from_arrays(domain, *_arrays(domain, rows))
    np.testing.assert_array_equal(tpe.distinct_rows(pool), config_first(rows))
    # every cached row is a history row
    losses = [None if t % 7 == 3 else float(t % 5) for t in range(len(seen))]  # (failed: seen too)
    trials = _trials_of(domain, seen, losses)
    want = config_first([pool.config(r) for r in range(300)],
                        [_doc_config(d) for d in trials.trials])
    assert (want < 0).any() and (want >= 0).any()
    np.testing.assert_array_equal(tpe.distinct_rows(pool, trials, domain), want)
    # a NaN loss drops its trial from the history (collect_history): a row list
    losses[5] = losses[20] = float("nan")
    trials = _trials_of(domain, seen, losses)
    hist = tpe.collect_history(trials, pool.labels)
    assert hist.tids.size == len(seen) - 2
    kept = [c for t, c in enumerate(seen) if t not in (5, 20)]
    np.testing.assert_array_equal(tpe.distinct_rows(pool, trials), config_first(rows, kept))


def fifteen(hp_):
    """15 configurations: a choice of three quantized labels of five values."""
    return hp_.choice("c", [hp_.quniform("q%d" % i, 0, 4, 1) for i in range(3)])


def _fifteen_history():
    """25 trials over 9 of the 15 configurations (q < 3 in every branch)."""
    domain = Domain(lambda x: 0, fifteen(hp))
    rng = np.random.RandomState(5)
    nine = [{"c": c, "q%d" % c: float(q)} for c in range(3) for q in range(3)]
    configs = nine + [nine[i] for i in rng.randint(0, 9, 16)]
    losses = [c["c"] + abs(c["q%d" % c["c"]] - 1.0) + 0.01 * t for t, c in enumerate(configs)]
    return domain, _trials_of(domain, configs, losses), nine


def test_distinct_rows_sampled_pool():
    domain, trials, nine = _fifteen_history()
    pool = tpe.Pool.sample(domain, trials, 3, 257)
    first = tpe.distinct_rows(pool, trials)
    want = config_first([pool.config(r) for r in range(257)],
                        [_doc_config(d) for d in trials.trials])
    np.testing.assert_array_equal(first, want)
    assert (first < 0).any()


# -- 3. suggest_sampled(distinct=True) ---------------------------------------------------
SEED = 42


def test_suggest_sampled_distinct():
    domain, trials, nine = _fifteen_history()
    n, ids = 4097, list(range(100, 108))
    pool = tpe.Pool.sample(domain, trials, SEED, n)
    configs = [pool.config(r) for r in range(n)]
    first = config_first(configs, [_doc_config(d) for d in trials.trials])
    fresh = first == np.arange(n)
    assert 3 <= fresh.sum() <= 6  # (a seed that leaves fewer fresh classes shows nothing)
    rows = _expected_order(pool.scores(), ~fresh, 8)
    docs = tpe.suggest_sampled(ids, domain, trials, SEED, n_EI_candidates=n, n_startup_jobs=5,
                               distinct=True)
    got = [_doc_config(d) for d in docs]
    assert got == [configs[r] for r in rows]
    assert [d["tid"] for d in docs] == ids[:len(rows)]
    assert len({_ckey(c) for c in got}) == len(got) == fresh.sum()
    assert not {_ckey(c) for c in got} & {_ckey(c) for c in nine}
    # keep: a rejected row is still the first of its class
    keep = lambda cols: np.arange(len(cols["c"])) != rows[0]  # noqa: E731
    kept = tpe.suggest_sampled(ids, domain, trials, SEED, n_EI_candidates=n, n_startup_jobs=5,
                               distinct=True, keep=keep)
    assert [_doc_config(d) for d in kept] == [configs[r] for r in rows[1:]]


def test_suggest_sampled_distinct_startup():
    """Startup phase: the first fresh prior rows in row order."""
    domain, trials, nine = _fifteen_history()
    labels, draws = rand.draw_priors(domain, 9, 512)
    configs = rand._configs(domain, labels, draws)
    first = config_first(configs, [_doc_config(d) for d in trials.trials])
    rows = np.flatnonzero(first == np.arange(512))
    assert 3 <= rows.size <= 6
    docs = tpe.suggest_sampled([7, 8, 9], domain, trials, 9, n_EI_candidates=512,
                               n_startup_jobs=100, distinct=True)
    assert [_doc_config(d) for d in docs] == [configs[r] for r in rows[:3]]


# -- 4. no false positives end to end ----------------------------------------------------
def test_distinct_changes_nothing_on_a_continuous_space():
    space = {"x": hp.uniform("x", -1, 1), "c": hp.choice("c", [0, 1, 2])}
    trials = Trials()
    fmin(lambda p: p["x"] ** 2 + p["c"], space, algo=rand.suggest, max_evals=30, trials=trials,
         rstate=np.random.RandomState(1), show_progressbar=False)
    domain = Domain(lambda x: 0, space)
    ids = list(range(50, 58))
    kw = dict(n_EI_candidates=4097, n_startup_jobs=5)
    plain = tpe.suggest_sampled(ids, domain, trials, 3, **kw)
    off = tpe.suggest_sampled(ids, domain, trials, 3, distinct=False, **kw)
    on = tpe.suggest_sampled(ids, domain, trials, 3, distinct=True, **kw)
    assert len(plain) == 8
    assert [d["misc"] for d in off] == [d["misc"] for d in plain]
    assert [d["misc"] for d in on] == [d["misc"] for d in plain]


# -- 5. fmin stops on a used-up space ------------------------------------------------------
def test_fmin_stops_when_the_space_is_used_up():
    trials = Trials()
    fmin(lambda v: float(v), fifteen(hp),
         algo=partial(tpe.suggest_sampled, distinct=True, n_EI_candidates=1024, n_startup_jobs=5),
         max_evals=60, max_queue_len=4, trials=trials, rstate=np.random.RandomState(0),
         show_progressbar=False)
    assert 5 < len(trials) <= 15
    keys = [_ckey(_doc_config(d)) for d in trials.trials]
    assert len(set(keys)) == len(keys)


# -- 6. suggest_from_pool(distinct=True) ---------------------------------------------------
def test_suggest_from_pool_distinct():
    domain, trials, nine = _fifteen_history()
    every = [{"c": c, "q%d" % c: float(q)} for c in range(3) for q in range(5)]
    rng = np.random.RandomState(2)
    rows = [every[i] for i in rng.randint(0, 15, 120)]
    pool = tpe.Pool(domain, rows)
    first = config_first(rows, [_doc_config(d) for d in trials.trials])
    fresh = first == np.arange(120)
    assert fresh.sum() == 6  # 120 draws hold all 15 configurations
    S = tpe.score_configs(domain, trials, pool)
    kw = dict(pool=pool, n_startup_jobs=5, distinct=True)
    docs = tpe.suggest_from_pool([200, 201, 202, 203], domain, trials, 0, **kw)
    want = _expected_order(S, ~fresh, 4)
    assert [pool.row_of[t] for t in (200, 201, 202, 203)] == list(want)
    assert [_doc_config(d) for d in docs] == [rows[r] for r in want]
    taken = np.zeros(120, np.uint8)
    taken[want] = 1
    np.testing.assert_array_equal(pool.taken, taken)
    # the taken rows stay the first of their classes: two fresh rows are left
    more = tpe.suggest_from_pool([204, 205, 206], domain, trials, 0, **kw)
    rest = _expected_order(S, ~fresh | (taken != 0), 3)
    assert len(rest) == 2 and [pool.row_of[t] for t in (204, 205)] == list(rest)
    assert [_doc_config(d) for d in more] == [rows[r] for r in rest]
    assert tpe.suggest_from_pool([207], domain, trials, 0, **kw) == []
    assert pool.n_untaken == 114
    # startup phase: startup_rows over the fresh untaken rows
    pool2 = tpe.Pool(domain, rows)
    pool2.mark_taken([int(want[0])])
    docs = tpe.suggest_from_pool([300, 301], domain, trials, 4, pool=pool2, n_startup_jobs=100,
                                 distinct=True)
    picked = startup_rows(tpe.Pool(domain, rows), 4, 2,
                          stale=~fresh | (np.arange(120) == want[0]))
    assert [pool2.row_of[t] for t in (300, 301)] == list(picked)
    assert fresh[picked].all() and want[0] not in picked
    # without the keyword a repeated configuration can come back
    pool3 = tpe.Pool(domain, rows)
    plain = tpe.suggest_from_pool(list(range(400, 420)), domain, trials, 0, pool=pool3,
                                  n_startup_jobs=5)
    assert len({_ckey(_doc_config(d)) for d in plain}) < 20
    grid = tpe.GridPool(domain, {"c": [0, 1, 2], "q0": range(5), "q1": range(5), "q2": range(5)})
    with pytest.raises(ValueError, match="distinct by construction"):
        tpe.suggest_from_pool([1], domain, trials, 0, pool=grid, distinct=True)
    with pytest.raises(ValueError, match="distinct by construction"):
        tpe.distinct_rows(grid)
