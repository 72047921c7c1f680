"""tpe.Pool on the GPU: score_configs against the reference's own numbers and
the oracle, the fold's bits, tpe_pool_topk's order, and suggest_from_pool.

Tolerances: the project's fp64 log-density tolerance (test_gpu_parity.py: rtol
1e-6 per log-density), applied term-wise to the joint score:
|S_dev - S_ref| <= 1e-6 * sum_labels (|below_llik| + |above_llik|); orders and
the fold's bits are compared exactly.
"""
import ctypes
from functools import partial

import numpy as np
import pytest

from hyperopt_amd import STATUS_FAIL, STATUS_OK, Domain, Trials, fmin, hp, rand, tpe
from hyperopt_amd import _lib as L
from hyperopt_amd import pool as pool_mod
from hyperopt_amd.base import trials_from_docs
from oracle import tpe_oracle as O
from tests.golden import spaces
from tests.golden_io import load

pytestmark = pytest.mark.gpu

TILE = 4096  # rows per selection tile (csrc/tpe_pool.hip)
INT_KINDS = ("randint", "categorical")


def _trials_from_fixture(arrays, meta):
    # (as tests/test_host_api.py builds them)
    tids = arrays["hist_tids"]
    losses = arrays["hist_losses"]
    labels = sorted(meta["specs"])
    docs = []
    for tid, loss in zip(tids, losses):
        idxs, vals = {}, {}
        for lab in labels:
            oi = arrays["obs_idxs/" + lab]
            pos = np.nonzero(oi == tid)[0]
            idxs[lab] = [int(tid)] if pos.size else []
            vals[lab] = [float(arrays["obs_vals/" + lab][pos[0]])] if pos.size else []
        result = {"status": STATUS_OK, "loss": float(loss)} if np.isfinite(loss) else \
            {"status": STATUS_FAIL}
        docs.append({"state": 2, "tid": int(tid), "spec": None, "result": result,
                     "misc": {"tid": int(tid), "cmd": None, "workdir": None, "idxs": idxs,
                              "vals": vals},
                     "exp_key": None, "owner": None, "version": 0, "book_time": None,
                     "refresh_time": None})
    return trials_from_docs(docs), labels


_CASES = {}


def _case(name):
    """(arrays, meta, trials, domain) of an end-to-end fixture, built once."""
    if name not in _CASES:
        arrays, meta = load("e2e_" + name)
        trials, _ = _trials_from_fixture(arrays, meta)
        domain = Domain(lambda x: 0, spaces.SPACES[meta["space"]](hp))
        _CASES[name] = (arrays, meta, trials, domain)
    return _CASES[name]


def _expected_order(scores, taken, k):
    """The rule in numpy: untaken rows, NaN first, larger score first
    (-0.0 == +0.0), equal scores to the smaller row."""
    idx = np.flatnonzero(np.asarray(taken) == 0)
    s = np.asarray(scores, np.float64)[idx]
    nan = np.isnan(s)
    return idx[np.lexsort((idx, np.where(nan, 0.0, -s), ~nan))][:k]


def _topk(scores, taken, k, poison=-7):
    """tpe_pool_topk through the C ABI: (rows written, count)."""
    import torch
    lib = L.load()
    n = len(scores)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_s = torch.from_numpy(np.ascontiguousarray(scores, np.float64)).to(dev)
    d_t = torch.from_numpy(np.ascontiguousarray(taken, np.uint8)).to(dev)
    d_out = torch.full((max(min(k, n), 1),), poison, dtype=torch.int64, device=dev)
    d_cnt = torch.full((1,), poison, dtype=torch.int64, device=dev)
    need = lib.tpe_pool_topk_scratch_bytes(n, k)
    assert need > 0
    d_ws = torch.empty(need, dtype=torch.uint8, device=dev)
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(lib.tpe_pool_topk(d_s.data_ptr(), d_t.data_ptr(), n, k, d_out.data_ptr(),
                              d_cnt.data_ptr(), d_ws.data_ptr(), sp), "tpe_pool_topk")
    return d_out.cpu().numpy(), int(d_cnt.item())


def _fold_numpy(terms, active):
    s = np.zeros(terms.shape[0])
    for j in range(terms.shape[1]):  # sequential, in domain.params order
        s = np.where(active[:, j], s + terms[:, j], s)
    return s


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64),
                          np.asarray(b, np.float64).view(np.int64))


# -- 1. against the reference's own numbers -------------------------------------
@pytest.mark.parametrize("case", ["mixed_50d", "many_dists", "many_dists_pw", "quniform_ties"])
def test_scores_and_order_match_reference(case):
    arrays, meta, trials, domain = _case(case)
    labels = list(domain.params)
    n = meta["n_ei"]
    configs = []
    for i in range(n):
        cfg = {}
        for lab in labels:
            spec = domain.specs[lab]
            v = arrays["cand/" + lab][i]
            if spec.kind in INT_KINDS:
                low = int(spec.args[0]) if spec.kind == "randint" and len(spec.args) > 1 and \
                    spec.args[1] is not None else 0
                v = int(v) + low
            cfg[lab] = v
        configs.append(cfg)
    pool = tpe.Pool(domain, configs)
    bl = np.stack([arrays["bl/" + lab] for lab in labels], 1)
    al = np.stack([arrays["al/" + lab] for lab in labels], 1)
    s_ref = (bl - al).sum(1)
    assert np.isfinite(s_ref).all()
    gap = np.diff(np.sort(s_ref)).min()
    assert gap > 1e-5  # (the fixtures' rows are distinct: 7.2e-5 is the smallest gap)
    S, terms = tpe.score_configs(domain, trials, pool, prior_weight=meta["prior_weight"],
                                 gamma=meta["gamma"], return_terms=True)
    err = np.abs(S - s_ref)
    print(case, "max |S - S_ref| = %.3g, gap = %.3g" % (err.max(), gap))
    assert (err <= 1e-6 * (np.abs(bl) + np.abs(al)).sum(1)).all()
    assert (np.abs(terms - (bl - al)) <= 1e-6 * (np.abs(bl) + np.abs(al))).all()
    assert err.max() < gap / 2
    assert _same_bits(S, _fold_numpy(terms, pool.active))
    rows, count = _topk(S, np.zeros(n, np.uint8), n)
    assert count == n
    np.testing.assert_array_equal(rows, _expected_order(s_ref, np.zeros(n), n))


# -- 2. conditional spaces against the oracle -----------------------------------
@pytest.mark.parametrize("case", ["nested", "readme"])
def test_conditional_pool_matches_oracle(case, monkeypatch):
    arrays, meta, trials, domain = _case(case)
    labels = list(domain.params)
    rng = np.random.RandomState(11)
    pool = tpe.Pool(domain, [rand.sample_config(domain, rng) for _ in range(300)])
    assert 0 < pool.n_active.min() < 300  # rows differ in which labels are live
    S, terms = tpe.score_configs(domain, trials, pool, prior_weight=meta["prior_weight"],
                                 gamma=meta["gamma"], return_terms=True)
    assert terms.shape == (300, len(labels))
    np.testing.assert_array_equal(np.isnan(terms), ~pool.active)
    for j, lab in enumerate(labels):
        spec = domain.specs[lab]
        below, above = O.ap_split_trials(arrays["obs_idxs/" + lab], arrays["obs_vals/" + lab],
                                         arrays["hist_tids"], arrays["hist_losses"],
                                         meta["gamma"])
        a = pool.active[:, j]
        cand = pool.vals[a, j]
        with np.errstate(all="ignore"):
            if spec.kind in INT_KINDS:
                ref = O.categorical_label_scores(spec.kind, spec.args, below, above, cand,
                                                 prior_weight=meta["prior_weight"])
            else:
                ref = O.continuous_label_scores(spec.kind, spec.args, below, above, cand,
                                                prior_weight=meta["prior_weight"])
        rb, ra = ref["below_llik"], ref["above_llik"]
        err = np.abs(terms[a, j] - (rb - ra))
        assert (err <= 1e-6 * (np.abs(rb) + np.abs(ra))).all(), (lab, err.max())
    # -- 3. the fold's bits, in one chunk and in chunks of two labels
    assert _same_bits(S, _fold_numpy(terms, pool.active))
    monkeypatch.setattr(pool_mod, "CHUNK_ELEMS", 2 * len(pool))
    S2, terms2 = tpe.score_configs(domain, trials, pool, prior_weight=meta["prior_weight"],
                                   gamma=meta["gamma"], return_terms=True)
    assert _same_bits(S2, S) and _same_bits(terms2, terms)
    assert _same_bits(tpe.score_configs(domain, trials, pool, prior_weight=meta["prior_weight"],
                                        gamma=meta["gamma"]), S)


# -- 4. tpe_pool_topk alone -----------------------------------------------------
def _score_vector(n, rng, kind):
    if kind == "equal":
        return np.full(n, 1.25), np.zeros(n, np.uint8)
    s = np.round(rng.normal(size=n), 1)  # a few hundred distinct values: many duplicates
    taken = (rng.uniform(size=n) < 0.3).astype(np.uint8)
    if n >= 8:
        pos = rng.permutation(n)[:8]
        s[pos[0]] = s[pos[1]] = np.nan
        s[pos[2]] = s[pos[3]] = np.inf
        s[pos[4]] = -np.inf
        s[pos[5]], s[pos[6]] = -0.0, 0.0
        s[pos[7]] = 0.0
        taken[pos[[0, 2, 5, 6, 7]]] = 0
    if kind == "open":
        taken[:] = 0
    return s, taken


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 3 * TILE + 17])
def test_topk_order(n):
    rng = np.random.RandomState(n)
    for kind in ("holes", "open", "equal"):
        s, taken = _score_vector(n, rng, kind)
        free = int((taken == 0).sum())
        for k in sorted({0, 1, free, n, n + 5}):
            rows, count = _topk(s, taken, k)
            want = _expected_order(s, taken, k)
            assert count == want.size == min(k, free), (kind, k)
            np.testing.assert_array_equal(rows[:count], want, err_msg="%s k=%d" % (kind, k))
            assert (rows[count:] == -7).all()  # nothing written past the count
    # signed zeros tie by row, NaN first, whatever the sign bit of the NaN
    s = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -0.0, 1.0])[:max(1, min(n, 7))]
    rows, count = _topk(s, np.zeros(s.size, np.uint8), s.size)
    np.testing.assert_array_equal(rows, _expected_order(s, np.zeros(s.size), s.size))
    if s.size == 7:
        assert rows.tolist() == [2, 3, 4, 6, 0, 1, 5]


# -- 5. suggest_from_pool -------------------------------------------------------
def _draw_pool(domain, n, seed):
    rng = np.random.RandomState(seed)
    return tpe.Pool(domain, [rand.sample_config(domain, rng) for _ in range(n)])


def test_suggest_from_pool_ranks():
    _, meta, trials, domain = _case("many_dists")
    kw = dict(prior_weight=meta["prior_weight"], gamma=meta["gamma"])
    pool = _draw_pool(domain, 200, 5)
    S = tpe.score_configs(domain, trials, pool, **kw)
    order = _expected_order(S, np.zeros(200), 200)
    ids = trials.new_trial_ids(5)
    docs = tpe.suggest_from_pool(ids, domain, trials, 123, pool=pool, verbose=False, **kw)
    like = tpe.suggest(trials.new_trial_ids(1), domain, trials, 123, verbose=False, **kw)[0]
    assert len(docs) == 5
    for i, doc in enumerate(docs):
        cfg = pool.config(order[i])
        assert doc["tid"] == doc["misc"]["tid"] == ids[i]
        assert set(doc) == set(like) and set(doc["misc"]) == set(like["misc"])
        assert doc["misc"]["vals"] == {lab: [cfg[lab]] if lab in cfg else []
                                       for lab in domain.params}
        assert doc["misc"]["idxs"] == {lab: [ids[i]] if lab in cfg else []
                                       for lab in domain.params}
        assert pool.row_of[ids[i]] == order[i]
    assert pool.n_untaken == 195 and pool.taken[order[:5]].all()
    # the history is unchanged: the next ranks
    ids2 = trials.new_trial_ids(5)
    docs2 = tpe.suggest_from_pool(ids2, domain, trials, 7, pool=pool, verbose=False, **kw)
    assert [pool.row_of[t] for t in ids2] == order[5:10].tolist() and len(docs2) == 5
    # a released row is offered again, first if it is the best
    pool.release([order[0]])
    assert ids[0] not in pool.row_of
    doc = tpe.suggest_from_pool(trials.new_trial_ids(1), domain, trials, 7, pool=pool,
                                verbose=False, **kw)[0]
    assert pool.row_of[doc["tid"]] == order[0]
    # fewer untaken rows than ids, then none
    pool.mark_taken(np.delete(np.arange(200), order[[50, 60, 70]]))
    ids3 = trials.new_trial_ids(5)
    docs3 = tpe.suggest_from_pool(ids3, domain, trials, 7, pool=pool, verbose=False, **kw)
    assert [d["tid"] for d in docs3] == ids3[:3]
    assert [pool.row_of[t] for t in ids3[:3]] == order[[50, 60, 70]].tolist()
    assert tpe.suggest_from_pool(trials.new_trial_ids(2), domain, trials, 7, pool=pool,
                                 verbose=False, **kw) == []


def test_suggest_from_pool_startup():
    domain = Domain(lambda x: 0, spaces.SPACES["nested"](hp))

    def draw(seed):
        pool = _draw_pool(domain, 1000, 2)
        pool.mark_taken(np.arange(0, 1000, 3))
        before = pool.taken.copy()
        trials = Trials()
        docs = tpe.suggest_from_pool(trials.new_trial_ids(8), domain, trials, seed, pool=pool,
                                     n_startup_jobs=20, verbose=False)
        rows = [pool.row_of[d["tid"]] for d in docs]
        assert len(docs) == 8 and len(set(rows)) == 8 and not before[rows].any()
        assert pool.taken[rows].all()
        for d, r in zip(docs, rows):
            cfg = pool.config(r)
            assert {k: v[0] for k, v in d["misc"]["vals"].items() if v} == cfg
        return rows
    assert draw(4) == draw(4)
    assert draw(4) != draw(5)


def test_fmin_over_a_grid_pool():
    space = {"x": hp.quniform("x", 0, 40, 1), "y": hp.quniform("y", 0, 40, 1)}
    domain = Domain(lambda p: 0.0, space)
    grid = [{"x": float(x), "y": float(y)} for x in range(41) for y in range(41)]
    pool = tpe.Pool(domain, grid)
    trials = Trials()
    fmin(lambda p: (p["x"] - 13.0) ** 2 + (p["y"] - 29.0) ** 2, space,
         algo=partial(tpe.suggest_from_pool, pool=pool), max_evals=40, max_queue_len=4,
         trials=trials, rstate=np.random.RandomState(0), show_progressbar=False)
    assert len(trials) == 40 and len(pool.row_of) == 40
    rows = [pool.row_of[d["tid"]] for d in trials.trials]
    assert len(set(rows)) == 40 and pool.n_untaken == 41 * 41 - 40
    for d, r in zip(trials.trials, rows):  # every document is its pool row
        assert {k: v[0] for k, v in d["misc"]["vals"].items()} == grid[r]
    seen = {(d["misc"]["vals"]["x"][0], d["misc"]["vals"]["y"][0]) for d in trials.trials}
    assert len(seen) == 40
