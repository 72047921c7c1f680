"""The climb of joint.py "Refining" on the host: ``joint.refine_numpy`` against
the existing ``joint.score_numpy``, and the argument errors of ``refine=``.

A central difference of ``score_numpy`` in t, step delta, is the mean of g over
[t - delta, t + delta]: off g(t) by at most delta sup |J''|, and per set log L''
= -E_r[1 / sigma^2] + Var_r[(mu - t) / sigma^2], so |J''| <= 2 (1 / sigma^2 + R^2
/ sigma^4) (sigma: the label's smallest bandwidth, R: the largest |mu_i - t|).
delta = 1e-6 sigma; rounding adds 8 eps (|log L_below| + |log L_above|) / (2 delta).
"""
import numpy as np
import pytest

from hyperopt_amd import Domain, hp, tpe
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from tests import joint_util as U
from tests.refine_util import KW, all_kinds_case


def test_value_and_gradient_against_central_differences_of_score_numpy():
    domain, _trials, hist, vals = all_kinds_case()
    models = J.label_models(domain)
    cont = J.moving_labels(models)
    assert [models[d].label for d in cont] == ["c", "d", "g", "h"]
    out, J0, _J1, g, acc = J.refine_numpy(domain, hist, vals, 0, **KW)
    assert out.tobytes() == vals.tobytes() and out is not vals and not acc.any()  # the identity
    S, Lb, La = J.score_numpy(domain, hist, vals, return_parts=True, **KW)
    np.testing.assert_array_equal(np.flatnonzero(np.isnan(S)), [5, 9])
    fin = np.isfinite(S)
    assert (np.isnan(J0) == np.isnan(S)).all()
    assert (np.abs(J0 - S)[fin] <= 1e-12 * (np.abs(Lb) + np.abs(La))[fin]).all()
    cols = [m.col for m in models]
    sets = [J.set_rows(hist, mask, cols) for mask in J.split_sets(hist, KW["gamma"])]
    for j, d in enumerate(cont):
        m = models[d]
        sigma = min([m.sigma] + [J.bandwidths(models, r.size, KW["bandwidth"])[d] for r in sets])
        delta = 1e-6 * sigma
        t = J._fit(m, vals[:, m.col])
        mus = np.append(J._fit(m, np.asarray(hist.vals)[np.concatenate(sets), m.col]), m.mu)
        R = np.abs(t[:, None] - mus[None, :]).max(1) + delta
        side = []
        for sign in (1.0, -1.0):
            moved = vals.copy()
            moved[:, m.col] = np.exp(t + sign * delta) if m.is_log else t + sign * delta
            side.append(J.score_numpy(domain, hist, moved, **KW))
        err = np.abs((side[0] - side[1]) / (2.0 * delta) - g[:, j])
        tol = delta * 2.0 * (1.0 / sigma ** 2 + R ** 2 / sigma ** 4) + \
            8.0 * np.finfo(float).eps * (np.abs(Lb) + np.abs(La)) / (2.0 * delta)
        assert (err[fin] <= tol[fin]).all()


def test_argument_errors():
    domain, trials, hist, vals = all_kinds_case()
    for bad in (-1, 2.0, "3", True):
        for call in (lambda: J.refine_numpy(domain, hist, vals, bad),
                     lambda: tpe.refine_configs(domain, trials, vals, bad),
                     lambda: tpe.suggest_sampled([0], domain, trials, 0, joint=True, refine=bad)):
            with pytest.raises(ValueError, match="refine="):
                call()
    for joint in (False, "tree", "chain"):
        with pytest.raises(ValueError, match="refine= .* needs joint=True"):
            tpe.suggest_sampled([0], domain, trials, 0, joint=joint, refine=4)
    pool = tpe.Pool.from_arrays(domain, vals[:4], np.ones((4, vals.shape[1]), bool))
    with pytest.raises(ValueError, match="closed set"):
        tpe.suggest_from_pool([0], domain, trials, 0, pool=pool, joint=True, refine=4)
    flat = Domain(lambda x: 0, {"x": hp.uniform("x", 0, 1), "y": hp.uniform("y", 0, 1)})
    grid = tpe.GridPool(flat, {"x": [0.1, 0.5], "y": [0.2, 0.7]}, joint=True)
    with pytest.raises(ValueError, match="GridPool"):
        tpe.suggest_from_pool([0], flat, U.make_trials(flat, [], []), 0, pool=grid, joint=True,
                              refine=4)
    n = J._L.REFINE_MAX_CONT + 1  # one continuous label too many
    wide = Domain(lambda x: 0, {"x%02d" % i: hp.uniform("x%02d" % i, 0, 1) for i in range(n)})
    none = U.make_trials(wide, [], [])
    for call in (lambda: J.refine_numpy(wide, tpe.collect_history(none, list(wide.params)),
                                        np.full((1, n), 0.5), 1),
                 lambda: tpe.refine_configs(wide, none, np.full((1, n), 0.5), 1),
                 lambda: tpe.suggest_sampled([0], wide, none, 0, joint=True, refine=1)):
        with pytest.raises(ValueError, match="at most %d" % (n - 1)):
            call()


def test_refine_none_builds_the_calls_it_always_built(monkeypatch):
    """``refine=None`` (and 0): ``_sample``, ``_pick`` and ``take_rows`` with the
    arguments of the code before ``refine`` existed, and never the climb."""
    domain, trials, _hist, vals = all_kinds_case()
    calls = []

    class _Pool(object):
        n_untaken, vals, __len__ = 8, None, lambda self: 8
        mark_taken = lambda self, rows: calls.append(("taken", list(rows)))  # noqa: E731

    _Dev = type("_Dev", (), dict(rows_out="the rows on the device"))

    def step(name, result):
        def run(*args, **kw):
            calls.append((name, args, kw))
            return result
        return run

    def no_climb(*args, **kw):
        raise AssertionError("refine=None reached the climb")

    monkeypatch.setattr(pool_mod, "_sample", step("sample", _Pool()))
    monkeypatch.setattr(pool_mod, "_pick", step("pick", np.asarray([6, 2], np.int64)))
    monkeypatch.setattr(pool_mod, "take_rows",
                        step("take", (vals[:2], np.ones((2, vals.shape[1]), bool))))
    for mod, name, f in ((pool_mod, "_mirror", lambda pool, eng: _Dev),
                         (tpe, "engine", lambda: "eng"), (pool_mod, "_refine_rows", no_climb),
                         (J, "refine_device", no_climb)):
        monkeypatch.setattr(mod, name, f)
    for kw in (dict(), dict(refine=None), dict(refine=0)):
        del calls[:]
        docs = tpe.suggest_sampled([100, 101], domain, trials, 3, n_EI_candidates=8, joint=True,
                                   draw="joint", verbose=False, **dict(KW, **kw))
        assert len(docs) == 2 and [c[0] for c in calls] == ["sample", "pick", "take", "taken"]
        (_, args, skw), st = calls[0], calls[0][1][4]
        assert args[:4] == (domain, trials, 3, 8) and args[5] is False and set(skw) == {"hist"}
        assert (st.prior_weight, st.gamma, st.lf, st.lie, st.refine) == (0.7, 0.3, 25, None, 0)
        assert st.joint == dict(bandwidth=0.25, cat_smoothing=0.5, tree=False)
        pargs = calls[1][1]
        assert pargs[0] == "eng" and pargs[2] is _Dev and pargs[3] == 2 and pargs[5] is False
        assert pargs[6] is st and len(pargs) == 7 and not calls[1][2]
        assert calls[2][1][1:] == ("the rows on the device", 2)
