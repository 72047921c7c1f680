"""The liar batch on the host: ``joint.liar_numpy`` against the scalar
restatement (tests/liar_util.py), its edge rules, and the argument errors of
``batch="liar"``.

Tolerance: both sides are fp64 evaluations of the same formulas that differ
only in who rounds (numpy's vector log / exp / sum against libm's and a Python
loop), as in test_joint_host.py; S_k = S_0 - (U_k - U_0) inherits an absolute
error from each of the three, so 1e-9 (|U_k| + |U_0| + |S_0|) is orders above
the rounding and far below a wrong factor.
"""
import numpy as np
import pytest

from hyperopt_amd import Domain, hp, rand, tpe
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from tests import joint_util as U
from tests import liar_util as LU

KW = dict(prior_weight=0.7, gamma=0.3, bandwidth=0.25, cat_smoothing=0.5)
_SHARED = {}


def _domain(space):
    return Domain(lambda x: 0, space)


def _all_kinds():
    """(domain, trials, hist, pool values, S_0, A_0) of the all-kinds case:
    P = 60, 80 trials; built once."""
    if not _SHARED:
        domain = _domain(U.all_kinds_space(hp))
        labels = list(domain.params)
        rng = np.random.RandomState(5)
        configs = [rand.sample_config(domain, rng) for _ in range(80)]
        losses = rng.uniform(size=80)
        losses[11] = np.inf  # a failed trial sits above
        trials = U.make_trials(domain, configs, losses)
        rows = [rand.sample_config(domain, rng) for _ in range(60)]
        rows[5]["i"] = 2.0e6   # qnormal far tail: J is NaN
        rows[9]["k"] = 0       # the pchoice option of probability zero: J is NaN
        vals = np.asarray([[float(c[lab]) for lab in labels] for c in rows])
        hist = tpe.collect_history(trials, labels)
        S0, _below, A0 = J.score_numpy(domain, hist, vals, linear_forgetting=25,
                                       return_parts=True, **KW)
        _SHARED["case"] = (domain, trials, hist, vals, S0, A0)
    return _SHARED["case"]


def _numpy(k, **kw):
    domain, _trials, hist, vals, S0, A0 = _all_kinds()
    return J.liar_numpy(domain, hist, vals, k, S0=S0, A0=A0, linear_forgetting=25,
                        **dict(KW, **kw))


def test_liar_numpy_matches_scalar_restatement_all_kinds():
    domain, trials, _hist, vals, S0, A0 = _all_kinds()
    ref = LU.liar_reference(domain, trials, vals, S0, A0, 6, lie_weight=1.3, lf=25, **KW)
    rows, at, S_k = _numpy(6, lie_weight=1.3)
    assert ref["rows"][:2] == [5, 9]  # the NaN rows first, in row order
    assert len(ref["rows"]) == 6 and len(set(ref["rows"])) == 6
    assert rows.tolist() == ref["rows"]
    assert rows.dtype == np.int64 and at.shape == (6,) and S_k.shape == (60,)
    np.testing.assert_array_equal(np.isnan(S_k), np.isnan(ref["S_k"]))
    np.testing.assert_array_equal(np.flatnonzero(np.isnan(S_k)), [5, 9])
    fin = ~np.isnan(S_k)
    bound = 1e-9 * (np.abs(ref["U_k"]) + np.abs(ref["U_0"]) + np.abs(S0))
    assert (np.abs(S_k[fin] - ref["S_k"][fin]) <= bound[fin]).all()
    assert np.isnan(at[:2]).all()
    assert (np.abs(at[2:] - ref["S_at_pick"][2:]) <= bound[rows[2:]]).all()
    # the penalty is >= 0, and largest on the picks themselves
    assert (S_k[fin] <= S0[fin]).all() and (S_k[rows[2:]] < S0[rows[2:]]).all()


def test_k_one_is_the_argmax_of_S0():
    _domain_, _trials, _hist, _vals, S0, _A0 = _all_kinds()
    gone = np.zeros(60, np.uint8)
    gone[[5, 9]] = 1
    rows, at, S_k = _numpy(1, taken=gone)
    best = int(np.nanargmax(S0))
    assert rows.tolist() == [best]
    assert at[0] == S0[best]
    assert LU.first_row(list(S0), list(gone)) == best


def test_a_lie_without_mass_leaves_U():
    """Rows of a category the pick cannot reach (cat_smoothing 0: a miss is
    log 0) get c = -inf: their U and their S keep their bits."""
    domain = _domain({"a": hp.choice("a", [0, 1, 2]), "x": hp.uniform("x", 0, 1)})
    configs = [{"a": i % 3, "x": 0.1 + 0.04 * i} for i in range(20)]
    trials = U.make_trials(domain, configs, [float(i) for i in range(20)])
    labels = list(domain.params)
    rows = [{"a": i % 3, "x": 0.05 + 0.1 * (i // 3)} for i in range(24)]
    vals = np.asarray([[float(c[lab]) for lab in labels] for c in rows])
    hist = tpe.collect_history(trials, labels)
    kw = dict(prior_weight=1.0, gamma=0.25, bandwidth=0.2, cat_smoothing=0.0)
    S0, _b, A0 = J.score_numpy(domain, hist, vals, return_parts=True, **kw)
    got_rows, _at, S_1 = J.liar_numpy(domain, hist, vals, 1, S0=S0, A0=A0, **kw)
    p = int(got_rows[0])
    a_col = labels.index("a")
    same = vals[:, a_col] == vals[p, a_col]
    assert same.any() and (~same).any()
    assert (S_1[~same].view(np.uint64) == S0[~same].view(np.uint64)).all()
    assert (S_1[same] < S0[same]).all()
    ref = LU.liar_reference(domain, trials, vals, S0, A0, 1, lf=25, **kw)
    assert ref["rows"] == [p]
    assert (ref["U_k"][~same].view(np.uint64) == ref["U_0"][~same].view(np.uint64)).all()


def test_exact_twins_go_in_row_order():
    domain, _trials, hist, vals, S0, A0 = _all_kinds()
    best = int(np.nanargmax(S0))
    order = [r for r in range(60) if r not in (5, 9)]
    twin_vals = np.concatenate([vals[order], vals[[best]]])          # the twin is the last row
    twin_S = np.concatenate([S0[order], S0[[best]]])
    twin_A = np.concatenate([A0[order], A0[[best]]])
    first = order.index(best)
    rows, _at, S_2 = J.liar_numpy(domain, hist, twin_vals, 2, S0=twin_S, A0=twin_A,
                                  linear_forgetting=25, **KW)
    assert rows[0] == first and first < 58
    # twins keep equal bits after any pick (the lie is hardest on its own twin)
    assert S_2[58:].view(np.uint64) == S_2[first:first + 1].view(np.uint64)
    assert S_2[58] < twin_S[58]
    # ... so without the first the second leads
    gone = np.zeros(59, np.uint8)
    gone[order.index(best)] = 1
    assert J.liar_numpy(domain, hist, twin_vals, 1, taken=gone, S0=twin_S, A0=twin_A,
                        linear_forgetting=25, **KW)[0].tolist() == [58]


def test_masks_are_respected_and_k_is_capped():
    domain, trials, _hist, vals, S0, A0 = _all_kinds()
    free = _numpy(6)[0]
    taken = np.zeros(60, np.uint8)
    taken[free[:3]] = 1
    distinct = np.zeros(60, np.uint8)
    distinct[free[3:5]] = 1
    rows, _at, _S = _numpy(6, taken=taken, distinct=distinct)
    assert not set(rows.tolist()) & set(free[:5].tolist())
    ref = LU.liar_reference(domain, trials, vals, S0, A0, 6, gone=(taken | distinct), lf=25,
                            **KW)
    assert rows.tolist() == ref["rows"]
    # k > the rows that are left: that many picks
    taken = np.ones(60, np.uint8)
    taken[[3, 17, 44]] = 0
    rows, at, S_k = _numpy(8, taken=taken)
    assert sorted(rows.tolist()) == [3, 17, 44] and at.shape == (3,)
    assert _numpy(100)[0].size == 60
    for k in (0, -2):
        rows, at, S_k = _numpy(k)
        assert rows.size == 0 and at.size == 0
        assert (S_k.view(np.uint64) == S0.view(np.uint64)).all()
    assert _numpy(4, taken=np.ones(60, np.uint8))[0].size == 0


def test_argument_errors():
    domain, trials, hist, vals, _S0, _A0 = _all_kinds()
    labels = list(domain.params)
    pool = tpe.Pool.from_arrays(domain, vals[[0, 1, 2]], np.ones((3, len(labels)), bool))
    ids = [100, 101]
    for kw in (dict(batch="liar"),                      # joint=False
               dict(batch="liar", joint="tree"),
               dict(batch="kriging", joint=True),
               dict(batch="liar", joint=True, lie_weight=0.0),
               dict(batch="liar", joint=True, lie_weight=-1.0),
               dict(batch="liar", joint=True, lie_weight=float("nan")),
               dict(batch="liar", joint=True, lie_weight=float("inf"))):
        with pytest.raises(ValueError):
            tpe.suggest_from_pool(ids, domain, trials, 0, pool=pool, **kw)
        with pytest.raises(ValueError):
            tpe.suggest_sampled(ids, domain, trials, 0, **kw)
    with pytest.raises(ValueError, match="joint=True on a Pool"):
        tpe.suggest_from_pool(ids, domain, trials, 0, pool=pool, batch="liar")
    with pytest.raises(ValueError, match="joint=True on a Pool"):
        tpe.suggest_sampled(ids, domain, trials, 0, batch="liar", joint="tree")
    small = _domain({"a": hp.choice("a", [0, 1]), "q": hp.quniform("q", 0, 4, 1)})
    grid = tpe.GridPool(small, {"a": [0, 1], "q": [0, 1, 2]}, joint=True)
    none = U.make_trials(small, [], [])
    with pytest.raises(ValueError, match="GridPool"):
        tpe.suggest_from_pool(ids, small, none, 0, pool=grid, joint=True, batch="liar")
    with pytest.raises(ValueError, match="GridPool"):
        tpe.pick_batch(small, none, grid, 2)
    with pytest.raises(ValueError):
        tpe.pick_batch(domain, trials, pool, 2, lie_weight=0.0)
    with pytest.raises(ValueError):
        J.liar_numpy(domain, hist, vals, 2, lie_weight=0.0)


def test_batch_none_builds_the_call_it_always_built(monkeypatch):
    """``batch=None`` goes through ``_score_device`` and ``_topk_device`` with
    the arguments of the code before ``batch`` existed: no parts asked for,
    settings without a lie, the same mask."""
    domain, trials, _hist, vals, _S0, _A0 = _all_kinds()
    labels = list(domain.params)
    pool = tpe.Pool.from_arrays(domain, vals[:8], np.ones((8, len(labels)), bool))
    calls = []

    class _Dev(object):
        mask = "the distinct mask"

    def score(*args, **kw):
        calls.append(("score", args, kw))
        return "eng", _Dev

    def topk(*args):
        calls.append(("topk", args))
        return np.asarray([6, 2], np.int64)

    def no_liar(*args, **kw):
        raise AssertionError("batch=None reached the liar path")

    monkeypatch.setattr(pool_mod, "_score_device", score)
    monkeypatch.setattr(pool_mod, "_topk_device", topk)
    monkeypatch.setattr(pool_mod, "_distinct_device", lambda *a: calls.append(("distinct", a)))
    monkeypatch.setattr(pool_mod, "_liar_device", no_liar)
    for kw in (dict(), dict(batch=None, lie_weight=2.0)):
        del calls[:]
        pool.release(np.arange(8))
        docs = tpe.suggest_from_pool([100, 101], domain, trials, 0, pool=pool, prior_weight=0.7,
                                     gamma=0.3, joint=True, bandwidth=0.25, cat_smoothing=0.5,
                                     distinct=True, verbose=False, **kw)
        assert [pool.row_of[i] for i in (100, 101)] == [6, 2] and len(docs) == 2
        assert [c[0] for c in calls] == ["score", "distinct", "topk"]
        _, args, skw = calls[0]
        assert args[:2] == (domain, trials) and args[2] is pool
        st = args[3]
        assert (st.prior_weight, st.gamma, st.lf, st.lie) == (0.7, 0.3, 25, None)
        assert args[4:] == (False,)
        assert set(skw) == {"hist"}
        assert st.joint == dict(bandwidth=0.25, cat_smoothing=0.5, tree=False)
        assert calls[2][1] == ("eng", _Dev, 8, 2, "the distinct mask")
