"""anneal.suggest on the GPU (tpe_anneal_sample): the ranked selection against
numpy's stable argsort, the concentrated draws against the numpy formulas,
distributions against the reference's own suggestions (tests/golden/
make_anneal_golden.py), the chain of picks on a nested space, determinism, the
incremental loss upload, and the drop-in API."""
import numpy as np
import pytest
from scipy import stats

from tests import golden_io
from tests.anneal_util import domain_of, history_docs, make_trials
from tests.golden import anneal_spaces, spaces

pytestmark = pytest.mark.gpu

P_MIN = 1e-4  # the threshold of the prior tests (test_gpu_prior.py)
DEVICE_SEED = 20240  # fixed before the first run


def _chi2(a, b):
    """Two-sample chi^2 p-value of two integer samples (test_gpu_prior._chi2)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    lo, hi = min(a.min(), b.min()), max(a.max(), b.max())
    ca = np.bincount(a - lo, minlength=hi - lo + 1)
    cb = np.bincount(b - lo, minlength=hi - lo + 1)
    keep = (ca + cb) >= 20
    table = np.vstack([np.append(ca[keep], ca[~keep].sum()), np.append(cb[keep], cb[~keep].sum())])
    table = table[:, table.sum(0) > 0]
    if table.shape[1] < 2:
        return 1.0
    return stats.chi2_contingency(table)[1]


def _device(dom, trials, ids, seed, avg_best_idx=2.0, shrink_coef=0.1):
    """(configs, [(labels per trial, debug records)] per level) of the device path."""
    from hyperopt_amd import anneal
    docs, col = anneal._columnar(dom, trials)
    assert anneal._cache_is_history(docs, col)
    trace = []
    configs = anneal._device_configs(list(ids), dom, col, seed, avg_best_idx, shrink_coef, trace)
    return configs, trace


def _by_label(trace_level, labels):
    """{label: debug records of its items, in trial order} of one level."""
    todo, dbg = trace_level
    flat = [lab for it in todo for lab in it]
    return {lab: dbg[[i for i, l in enumerate(flat) if l == lab]] for lab in labels}


# ---------------------------------------------------------------------------
# 5. selection
# ---------------------------------------------------------------------------
def _losses(rng, n):
    x = rng.normal(size=n).round(1)  # many exact ties, negatives
    for value in (0.0, -0.0, np.inf, -np.inf, np.nan, 2.5):
        x[rng.rand(n) < 0.06] = value
    return x


@pytest.mark.parametrize("avg_best_idx", [2.0, 1000.0])
@pytest.mark.parametrize("n_rows", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_selection_matches_stable_argsort(n_rows, avg_best_idx):
    from hyperopt_amd import _lib as L
    from hyperopt_amd import anneal, tpe
    from hyperopt_amd.engine import DeviceHistory
    rng = np.random.RandomState(n_rows)
    eng = tpe.engine()
    losses = _losses(rng, n_rows)
    active = np.zeros((n_rows, 3), bool)
    active[:, 0] = True            # full
    active[::3, 1] = True          # every third row
    active[rng.choice(n_rows, min(3, n_rows), replace=False), 2] = True  # three rows only
    vals = np.where(active, rng.uniform(0, 1, active.shape), np.nan)
    dh = DeviceHistory(eng, 3, cap=16)
    dh.append(vals, active)
    loss = eng.torch.from_numpy(losses).to(dh.device)
    rec = np.zeros(3, L.ANNEAL_DTYPE)
    rec["kind"], rec["a"], rec["b"] = L.PRIOR_UNIFORM, 0.0, 1.0
    rec["col"] = np.arange(3)
    rec["n_active"] = active.sum(0)
    rec["shrink"] = 1.0 / (1.0 + 0.1 * rec["n_active"])
    rec["key"] = tpe.label_keys_array(7, ["a", "b", "c"])
    n_trials = 192
    ids = np.arange(1000, 1000 + n_trials)
    items = [[t % 3] for t in range(n_trials)]  # one label per trial: every item is a new pick
    state = anneal.chain_state(eng, dh, rec, np.zeros(1), ids)
    out, dbg = anneal.sample_level(eng, dh, loss, rec, None, items, ids, avg_best_idx, state,
                                   debug=True)
    assert state["err"] == 0
    deep = 0
    for t in range(n_trials):
        j = t % 3
        rows = np.flatnonzero(active[:, j])
        order = np.argsort(losses[rows], kind="stable")
        g = int(dbg["g"][t])
        assert 0 <= g < rows.size and dbg["reused"][t] == 0
        assert dbg["row"][t] == rows[order[g]], (t, j, g)
        deep += g == rows.size - 1
        assert 0.0 <= out[t] <= 1.0
    if avg_best_idx > 2:
        assert deep >= n_trials // 3  # the three-row column always clips at T - 1
    # a wrong host count is flagged (a flag in a buffer), and the pick stays inside the rows found
    if n_rows > 3:
        bad = rec.copy()
        bad["n_active"][0] -= 1  # too few for the full column
        bad["n_active"][2] += 1  # too many for the three-row column
        state = anneal.chain_state(eng, dh, bad, np.zeros(1), ids)
        state["allow_err"] = True
        out2, dbg2 = anneal.sample_level(eng, dh, loss, bad, None, items, ids, avg_best_idx, state,
                                         debug=True)
        assert state["err"] == 4
        assert np.all(dbg2["g"][0::3] <= n_rows - 2) and np.all(dbg2["g"][2::3] <= 2)
        assert np.all(active[dbg2["row"], np.arange(n_trials) % 3])
        np.testing.assert_array_equal(dbg2["row"][1::3], dbg["row"][1::3])
        with pytest.raises(L.TpeHipError):
            state = anneal.chain_state(eng, dh, bad, np.zeros(1), ids)
            anneal.sample_level(eng, dh, loss, bad, None, items, ids, avg_best_idx, state)


# ---------------------------------------------------------------------------
# shared runs on the flat fixture
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flat_run():
    from hyperopt_amd import hp
    arrays, meta = golden_io.load("anneal_flat")
    dom = domain_of(anneal_spaces.flat(hp))
    trials = make_trials(dom, meta["labels"], arrays["hist"], arrays["losses"])
    ids = list(range(meta["first_id"], meta["first_id"] + 2000))
    configs, trace = _device(dom, trials, ids, DEVICE_SEED)
    assert len(trace) == 1  # a flat space is one level
    return dict(arrays=arrays, meta=meta, dom=dom, trials=trials, ids=ids, configs=configs,
                dbg=_by_label(trace[0], list(dom.params)))


def _ulps(x, n=8):
    return n * np.spacing(np.abs(x))


# ---------------------------------------------------------------------------
# 6. parameters and values of the concentrated draws
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", anneal_spaces.KINDS)
def test_parameters_and_values(flat_run, kind):
    r = flat_run
    spec = r["dom"].specs[kind]
    a = spec.args
    j = r["meta"]["labels"].index(kind)
    d = r["dbg"][kind]
    T = 60
    shrink = 1.0 / (1.0 + T * 0.1)
    val = r["arrays"]["hist"][d["row"], j]
    got = np.array([c[kind] for c in r["configs"]], dtype=np.float64)
    u = d["variate"]
    q = a[2] if kind.startswith("q") else None
    with np.errstate(all="ignore"):
        if kind in ("uniform", "quniform", "loguniform", "qloguniform"):
            low, high = float(a[0]), float(a[1])
            mid = np.log(val) if "log" in kind else val
            half = 0.5 * ((high - low) * shrink)
            mid = np.clip(mid, low + half, high - half)
            scale = np.maximum(np.maximum(abs(low), abs(high)), np.abs(mid))
            assert np.all(np.abs(d["p0"] - mid) <= _ulps(scale))
            assert np.all(np.abs(d["p1"] - half) <= _ulps(scale))
            assert np.all((u >= 0) & (u < 1))
            lo, hi = d["p0"] - d["p1"], d["p0"] + d["p1"]
            want = lo + (hi - lo) * u
            support = (low, high)
            if "log" in kind:
                want, support = np.exp(want), (np.exp(low), np.exp(high))
        elif kind in ("normal", "qnormal", "lognormal", "qlognormal"):
            mu = {"lognormal": np.log(val), "qlognormal": np.log(1e-16 + val)}.get(kind, val)
            sigma = float(a[1]) * shrink
            assert np.all(np.abs(d["p0"] - mu) <= _ulps(mu))
            assert np.all(np.abs(d["p1"] - sigma) <= _ulps(sigma))
            want = d["p0"] + d["p1"] * u
            support = (-np.inf, np.inf)
            if "log" in kind:
                want, support = np.exp(want), (0.0, np.inf)
        else:
            if kind == "pchoice":
                low, prior = 0, np.asarray(a[0], dtype=np.float64).reshape(-1)
            else:
                low, high = (0, int(a[0])) if a[1] is None else (int(a[0]), int(a[1]))
                prior = np.full(high - low, 1.0 / (high - low))
            K = prior.size
            assert np.array_equal(d["p0"], val - low) and np.all(d["p1"] == shrink)
            want = np.zeros(len(u))
            for i in range(len(u)):
                p = (1 - shrink) * (np.arange(K) == int(val[i]) - low) + shrink * prior
                c = np.cumsum(p)
                hit = np.flatnonzero(c[:-1] > u[i] * c[-1])
                want[i] = low + (hit[0] if hit.size else K - 1)
            support = (low, low + K - 1)
    if q is not None:
        want = np.round(want / q) * q
        support = (np.round(support[0] / q) * q, np.round(support[1] / q) * q)
    if q is not None or kind.startswith(("randint", "pchoice")):
        np.testing.assert_array_equal(got, want)
    else:
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    assert np.all((got >= support[0]) & (got <= support[1])), (got.min(), got.max(), support)
    if kind.startswith(("randint", "pchoice")):
        assert all(isinstance(c[kind], int) for c in r["configs"])


# ---------------------------------------------------------------------------
# 7. distributions against the reference
# ---------------------------------------------------------------------------
def test_distributions_match_reference(flat_run):
    r = flat_run
    arrays, labels = r["arrays"], r["meta"]["labels"]
    rank_of_row = np.empty(60, np.int64)
    rank_of_row[np.argsort(arrays["losses"], kind="stable")] = np.arange(60)
    first = list(r["dom"].params)[0]  # the label that makes the pick
    picks = r["dbg"][first]
    assert np.all(picks["reused"] == 0)
    for lab in labels:
        if lab != first:  # every other label reuses the one pick
            assert np.all(r["dbg"][lab]["reused"] == 1)
            np.testing.assert_array_equal(r["dbg"][lab]["row"], picks["row"])
    dev_rank = rank_of_row[picks["row"]]
    np.testing.assert_array_equal(dev_rank, picks["g"])
    ref_rank = rank_of_row[arrays["tids"]]  # (tid == row in the fixture's history)
    p = _chi2(dev_rank, ref_rank)
    assert p > P_MIN, ("rank", p)
    # g ~ geometric(1/2) - 1
    g = np.minimum(picks["g"], 7)
    expect = np.append(0.5 ** np.arange(1, 8), 0.5 ** 7) * len(g)
    p = stats.chisquare(np.bincount(g, minlength=8), expect).pvalue
    assert p > P_MIN, ("geometric", p)
    # values, among the calls that picked the best trial
    dev_best, ref_best = dev_rank == 0, ref_rank == 0
    assert dev_best.sum() > 800 and ref_best.sum() > 800
    qs = {"quniform": 3, "qloguniform": 2, "qnormal": 2, "qlognormal": 0.5, "randint10": 1,
          "randint12_25": 1, "pchoice": 1}
    for j, lab in enumerate(labels):
        x = np.array([c[lab] for c in r["configs"]], dtype=np.float64)[dev_best]
        y = arrays["vals"][ref_best, j]
        if lab in qs:
            p = _chi2(np.round(x / qs[lab]), np.round(y / qs[lab]))
        else:
            p = stats.ks_2samp(x, y).pvalue
        assert p > P_MIN, (lab, p)
        # the value variates: uniform, or standard normal
        v = r["dbg"][lab]["variate"]
        cdf = stats.norm.cdf if "normal" in lab else stats.uniform.cdf
        p = stats.kstest(v, cdf).pvalue
        assert p > P_MIN, (lab, "variate", p)


# ---------------------------------------------------------------------------
# 8. nested space: the chain of picks
# ---------------------------------------------------------------------------
def test_nested_chain_and_distributions():
    from hyperopt_amd import hp
    arrays, meta = golden_io.load("anneal_nested")
    labels = meta["labels"]
    dom = domain_of(spaces.nested(hp))
    hist = arrays["hist"]
    trials = make_trials(dom, labels, hist, arrays["losses"])
    ids = list(range(meta["first_id"], meta["first_id"] + 2000))
    configs, trace = _device(dom, trials, ids, DEVICE_SEED + 1)
    active = ~np.isnan(hist)
    col = {lab: j for j, lab in enumerate(labels)}
    branch = {0: {"lin_lr"}, 1: {"tree_depth", "tree_split"}, 2: {"nn_units", "nn_drop"}}
    live = np.zeros(len(ids), np.int64)
    for i, c in enumerate(configs):
        want = {"root"} | branch[c["root"]]
        if c["root"] == 1:
            want |= {"gini_w"} if c["tree_split"] == 0 else {"ent_w", "ent_s"}
        assert set(c) == want
        live[i] = sum(1 << col[lab] for lab in c)
    assert set(np.unique(live)) <= set(np.unique(arrays["live"]))
    # the chain, replayed from the debug records
    chains = [[] for _ in ids]
    for todo, dbg in trace:
        k = 0
        for chain, it in zip(chains, todo):
            for lab in it:
                d, j = dbg[k], col[lab]
                k += 1
                have = [r for r in chain if active[r, j]]
                if d["reused"]:
                    assert have and d["row"] == have[0]
                else:
                    assert not have and active[d["row"], j]
                    chain.append(int(d["row"]))
    n_picks = np.array([len(c) for c in chains])
    p = _chi2(n_picks, arrays["n_picks"])
    assert p > P_MIN, ("picks", p)
    p = _chi2([c["root"] for c in configs], arrays["root"])
    assert p > P_MIN, ("root", p)


# ---------------------------------------------------------------------------
# 9. determinism
# ---------------------------------------------------------------------------
def test_suggestion_is_a_function_of_seed_id_history(flat_run):
    from hyperopt_amd import anneal
    r = flat_run
    ids = r["ids"][:1000]
    docs = anneal.suggest(ids, r["dom"], r["trials"], DEVICE_SEED)
    again = anneal.suggest(ids, r["dom"], r["trials"], DEVICE_SEED)
    assert [d["misc"] for d in docs] == [d["misc"] for d in again]
    assert [d["misc"]["vals"] for d in docs] == \
        [{lab: [c[lab]] for lab in r["dom"].params} for c in r["configs"][:1000]]
    for i in (0, 1, 499, 640, 999):
        (one,) = anneal.suggest([ids[i]], r["dom"], r["trials"], DEVICE_SEED)
        assert one["misc"] == docs[i]["misc"]
    other = anneal.suggest(ids[:50], r["dom"], r["trials"], DEVICE_SEED + 1)
    assert [d["misc"]["vals"] for d in other] != [d["misc"]["vals"] for d in docs[:50]]
    idxs, vals = anneal.suggest_batch(ids[:20], r["dom"], r["trials"], DEVICE_SEED)
    assert vals["uniform"] == [d["misc"]["vals"]["uniform"][0] for d in docs[:20]]
    assert idxs["uniform"] == ids[:20]


# ---------------------------------------------------------------------------
# 10. a loss that arrives late; growth of the history and the loss vector
# ---------------------------------------------------------------------------
def test_late_loss_and_growth():
    from hyperopt_amd import JOB_STATE_DONE, JOB_STATE_NEW, hp
    dom = domain_of({"x": hp.uniform("x", 0, 1), "k": hp.randint("k", 5)})
    labels = ["x", "k"]
    rng = np.random.RandomState(3)

    def rows(n):
        return np.column_stack([rng.uniform(0, 1, n), rng.randint(5, size=n)]).astype(float)

    losses = rng.uniform(1, 2, 50).round(2)
    trials = make_trials(dom, labels, rows(50), losses)
    (late,) = history_docs(dom, trials, labels, rows(1), [np.nan], first_tid=50)
    late["state"], late["result"] = JOB_STATE_NEW, {"status": "new"}
    trials.insert_trial_docs([late])
    trials.refresh()
    late = trials.trials[50]
    ids = list(range(100, 300))

    def picks(avg):
        _, trace = _device(dom, trials, ids, 11, avg_best_idx=avg)
        d = _by_label(trace[0], list(dom.params))[list(dom.params)[0]]
        return d["row"], d["g"]

    def check_ranks(all_losses):
        row, g = picks(2.0)
        order = np.argsort(all_losses, kind="stable")
        np.testing.assert_array_equal(row, order[g])
        return row, g

    row, g = check_ranks(np.append(losses, np.inf))
    assert np.all(row[g == 0] != 50) and (g == 0).sum() > 50
    late["result"] = {"status": "ok", "loss": -100.0}  # fmin's order: result, then state
    late["state"] = JOB_STATE_DONE
    row, g = picks(1.0)
    assert np.all(g == 0) and np.all(row == 50)
    all_losses = np.append(losses, -100.0)
    check_ranks(all_losses)
    more = rng.uniform(0, 3, 3000).round(3)
    trials.insert_trial_docs(history_docs(dom, trials, labels, rows(3000), more, first_tid=51))
    trials.refresh()
    row, g = picks(1.0)
    assert np.all(row == 50)
    row, g = check_ranks(np.append(all_losses, more))
    assert row.max() > 50  # (the appended rows are picked too)


# ---------------------------------------------------------------------------
# 11. drop-in
# ---------------------------------------------------------------------------
def _loss(p):
    return float(np.sin(p["c"]) + 0.1 * p["b"] + np.log(p["h"]) ** 2 + 0.01 * p["i"])


@pytest.mark.parametrize("queue", [1, 4])
def test_fmin_anneal_and_mix(queue):
    from hyperopt_amd import Trials, anneal, fmin, hp, mix, partial, rand, tpe
    space = spaces.many_dists(hp)
    algos = [anneal.suggest,
             partial(mix.suggest, p_suggest=[(.1, rand.suggest), (.2, anneal.suggest),
                                             (.7, tpe.suggest)])]
    for algo in algos:
        trials = Trials()
        best = fmin(_loss, space, algo=algo, max_evals=60, trials=trials, max_queue_len=queue,
                    rstate=np.random.RandomState(5), show_progressbar=False)
        assert len(trials.trials) == 60 and set(best) == set(space)
        for d in trials.trials:
            trials.assert_valid_trial(d)
            assert all(len(v) == 1 for v in d["misc"]["vals"].values())
    # annealing concentrates: the late trials of the pure run sit nearer the best
    losses = np.array([t["result"]["loss"] for t in trials.trials])
    assert np.isfinite(losses).all()


class RefShapedTrials(object):
    """The reference Trials' document handling only (no columnar cache)."""

    def __init__(self):
        self._dynamic_trials = []
        self._trials = []

    def refresh(self):
        self._trials = [t for t in self._dynamic_trials if t["state"] in (0, 1, 2)]

    @property
    def trials(self):
        return self._trials

    def new_trial_docs(self, tids, specs, results, miscs):
        from hyperopt_amd import Trials
        return Trials.new_trial_docs(self, tids, specs, results, miscs)

    _exp_key = None


def test_anneal_over_foreign_trials(monkeypatch):
    from hyperopt_amd import JOB_STATE_DONE, anneal, hp
    calls = []
    real = anneal._device_configs
    monkeypatch.setattr(anneal, "_device_configs",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    dom = domain_of(spaces.many_dists(hp))
    ft = RefShapedTrials()
    for tid in range(30):
        (doc,) = anneal.suggest([tid], dom, ft, 100 + tid)
        vals = {k: v[0] for k, v in doc["misc"]["vals"].items()}
        doc["result"] = {"status": "ok", "loss": _loss(vals)}
        doc["state"] = JOB_STATE_DONE
        ft._dynamic_trials.append(doc)
        ft.refresh()
    assert len(calls) == 30 and len(ft.trials) == 30
    host = anneal.suggest_host([30], dom, ft, 1)
    assert set(host[0]["misc"]["vals"]) == set(dom.params)
