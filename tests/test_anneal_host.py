"""anneal.suggest_host / mix.suggest against the reference's own suggestions
(tests/golden/make_anneal_golden.py), the C ABI of tpe_anneal_sample without a
GPU, and the host path through fmin -- all CPU."""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _lib as L
from hyperopt_amd import Trials, anneal, fmin, hp, mix
from tests import golden_io
from tests.anneal_util import domain_of, make_trials
from tests.golden import anneal_spaces, spaces


# ---------------------------------------------------------------------------
# 1. suggest_host == the reference on single-label spaces
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", anneal_spaces.KINDS)
def test_suggest_host_matches_reference(kind):
    """Same RandomState stream, same picks: for both parameter sets and all 64
    ids the chosen tid is the reference's and so is the value (integers and
    lattice values exactly, floats to libm differences)."""
    arrays, meta = golden_io.load("anneal_single")
    dom = domain_of(anneal_spaces.single(hp, kind))
    trials = make_trials(dom, ["x"], arrays["hist/" + kind], arrays["losses"])
    for k, kw in enumerate(meta["psets"]):
        trace = []
        configs = anneal._host_configs(meta["new_ids"], dom, trials, meta["seed"],
                                       kw["avg_best_idx"], kw["shrink_coef"], trace)
        tids = np.array([t[0] for t in trace])
        np.testing.assert_array_equal(tids, arrays["tid/%s/%d" % (kind, k)])
        got = np.array([c["x"] for c in configs], dtype=np.float64)
        want = arrays["val/%s/%d" % (kind, k)]
        if kind.startswith(("randint", "pchoice")):
            assert all(isinstance(c["x"], int) for c in configs)
            np.testing.assert_array_equal(got, want)
        else:
            np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
        docs = anneal.suggest_host(meta["new_ids"][:3], dom, trials, meta["seed"], **kw)
        assert [d["misc"]["vals"]["x"][0] for d in docs] == [c["x"] for c in configs[:3]]


# ---------------------------------------------------------------------------
# 2. mix.suggest == the reference
# ---------------------------------------------------------------------------
def test_mix_matches_reference():
    arrays, meta = golden_io.load("mix_choices")
    stubs = [(p, (lambda k: lambda new_ids, domain, trials, seed: (k, int(seed)))(k))
             for k, p in enumerate(meta["p"])]
    got = np.array([mix.suggest([0], None, None, s, stubs) for s in meta["seeds"]])
    np.testing.assert_array_equal(got[:, 0], arrays["chosen"])
    np.testing.assert_array_equal(got[:, 1], arrays["passed"])
    assert len(set(got[:, 0])) == 3
    with pytest.raises(ValueError):
        mix.suggest([0], None, None, 0, [(0.2, stubs[0][1]), (0.7, stubs[1][1])])


# ---------------------------------------------------------------------------
# 3. the C ABI without a GPU
# ---------------------------------------------------------------------------
def _call(lib, rec, **kw):
    one = ctypes.c_void_p(8)  # a non-null stand-in: validation fails before any launch
    a = dict(vals=one, active=one, ld=16, n_cols=2, n_rows=10, loss=one, recs=one,
             host_recs=rec.ctypes.data_as(ctypes.c_void_p), n_recs=len(rec), p=one, item_off=one,
             item_label=one, n_items=3, new_ids=one, n_trials=2, avg_best_idx=2.0, chain=one,
             chain_n=one, chain_ld=len(rec), out=one, dbg=None, err=one, stream=None)
    a.update(kw)
    return lib.tpe_anneal_sample(*a.values())


def test_anneal_abi_without_gpu():
    lib = L.load()
    assert hasattr(lib, "tpe_anneal_sample")
    sizes = (ctypes.c_int32 * 2)()
    assert lib.tpe_anneal_struct_sizes(ctypes.cast(sizes, ctypes.c_void_p), 2) == 2
    assert tuple(sizes) == (L.ANNEAL_DTYPE.itemsize, L.ANNEAL_DBG_DTYPE.itemsize) == (64, 40)
    rec = np.zeros(1, L.ANNEAL_DTYPE)
    rec["b"], rec["shrink"], rec["n_active"] = 1.0, 0.5, 10
    assert _call(lib, rec, n_trials=0) == 0  # nothing to do
    assert _call(lib, rec, n_items=0) == 0
    cases = [(dict(kind=9), b"kind 9"),
             (dict(kind=L.PRIOR_RANDINT, a=3.0, b=3.0), b"high <= low"),
             (dict(kind=L.PRIOR_CATEGORICAL, n_cat=0), b"categorical"),
             (dict(col=2), b"column 2"), (dict(col=-1), b"column -1"),
             (dict(n_active=11), b"n_active 11")]
    for fields, text in cases:
        bad = rec.copy()
        for f, v in fields.items():
            bad[f] = v
        assert _call(lib, bad) == -1 and text in lib.tpe_last_error(), fields
    bad = rec.copy()
    bad["kind"], bad["n_cat"] = L.PRIOR_CATEGORICAL, 3
    assert _call(lib, bad, p=None) == -1 and b"categorical" in lib.tpe_last_error()
    for kw in (dict(n_trials=-1), dict(n_items=-2), dict(n_rows=-1), dict(ld=9), dict(n_recs=-1),
               dict(host_recs=None)):
        assert _call(lib, rec, **kw) == -1 and b"bad arguments" in lib.tpe_last_error(), kw
    for bad_avg in (0.0, -1.0, float("nan")):
        assert _call(lib, rec, avg_best_idx=bad_avg) == -1
        assert b"avg_best_idx" in lib.tpe_last_error()
    assert _call(lib, rec, chain_ld=0) == -1 and b"chain_ld" in lib.tpe_last_error()
    for name in ("vals", "active", "loss", "recs", "item_off", "item_label", "new_ids", "chain",
                 "chain_n", "out", "err"):
        assert _call(lib, rec, **{name: None}) == -1, name
        assert b"null pointer" in lib.tpe_last_error(), name
    big = 1 << 31
    assert _call(lib, rec, n_trials=big) == -3 and b"too large" in lib.tpe_last_error()
    assert _call(lib, rec, n_rows=big, ld=big) == -3 and b"too large" in lib.tpe_last_error()


# ---------------------------------------------------------------------------
# 4. the host path through fmin, and the fallback of anneal.suggest
# ---------------------------------------------------------------------------
def _leaves(x):
    if isinstance(x, dict):
        for k in sorted(x):
            yield from _leaves(x[k])
    elif isinstance(x, (int, float)) and not isinstance(x, bool):
        yield float(x)


def _objective(point):
    return float(np.sum(np.sin(1.3 * np.array(list(_leaves(point))))))


def _check_nested(trials, n):
    assert len(trials.trials) == n
    branch = {0: {"lin_lr"}, 1: {"tree_depth", "tree_split"}, 2: {"nn_units", "nn_drop"}}
    for d in trials.trials:
        trials.assert_valid_trial(d)
        vals = d["misc"]["vals"]
        live = {lab for lab, v in vals.items() if v}
        r = vals["root"][0]
        want = {"root"} | branch[r]
        if r == 1:
            want |= {"gini_w"} if vals["tree_split"][0] == 0 else {"ent_w", "ent_s"}
        assert live == want, (live, want)
        assert all(d["misc"]["idxs"][lab] == ([d["tid"]] if lab in live else [])
                   for lab in d["misc"]["idxs"])
        assert isinstance(r, int) and all(isinstance(vals[lab][0], float)
                                          for lab in live - {"root", "tree_split"})
    return [d["misc"]["vals"] for d in trials.trials]


def test_suggest_host_through_fmin():
    trials = Trials()
    fmin(_objective, spaces.nested(hp), algo=anneal.suggest_host, max_evals=40, trials=trials,
         rstate=np.random.RandomState(3), show_progressbar=False)
    _check_nested(trials, 40)
    assert len({d["misc"]["vals"]["root"][0] for d in trials.trials}) > 1


def test_from_tid_history_takes_the_host_path(monkeypatch):
    """A from_tid document (Ctrl.inject_results) makes the cached rows differ
    from the history: anneal.suggest must not touch the device path."""
    def no_device(*a, **k):
        raise AssertionError("device path taken")
    monkeypatch.setattr(anneal, "_device_configs", no_device)
    space = spaces.nested(hp)

    def seeded():
        trials = Trials()
        dom = domain_of(space)
        (src,) = anneal.suggest_host([0], dom, trials, 5)
        src["state"], src["result"] = 2, {"status": "ok", "loss": 1.0}
        trials.insert_trial_docs([src])
        trials.refresh()
        (more,) = anneal.suggest_host(trials.new_trial_ids(1), dom, trials, 6)
        (alias,) = trials.source_trial_docs([more["tid"]], [None], [{"status": "ok", "loss": 0.5}],
                                            [dict(more["misc"], cmd=None)], [trials.trials[0]])
        alias["state"] = 2
        trials.insert_trial_docs([alias])
        trials.refresh()
        assert trials.columnar(tuple(dom.params)).n_alias == 1
        return trials

    a, b = seeded(), seeded()
    fmin(_objective, space, algo=anneal.suggest, max_evals=40, trials=a,
         rstate=np.random.RandomState(4), show_progressbar=False)
    fmin(_objective, space, algo=anneal.suggest_host, max_evals=40, trials=b,
         rstate=np.random.RandomState(4), show_progressbar=False)
    assert _check_nested(a, 40) == _check_nested(b, 40)
    idxs, vals = anneal.suggest_batch([100, 101], domain_of(space), a, 9)
    docs = anneal.suggest_host([100, 101], domain_of(space), a, 9)
    assert vals["root"] == [d["misc"]["vals"]["root"][0] for d in docs]
    assert idxs["root"] == [100, 101]
