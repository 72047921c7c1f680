"""Per-label bandwidths on the host (joint.py, "Bandwidth per label"):
``loo_label_numpy`` against a plain double loop, its agreement with the scalar
curve, the mapping's bits, the rules of the choice, and the argument errors,
each raised before any engine exists."""
import math

import numpy as np
import pytest

from hyperopt_amd import hp, tpe
from hyperopt_amd import joint as J
from tests import joint_util as U
from tests.refine_util import random_case

KW = dict(prior_weight=0.7, gamma=1.2, linear_forgetting=4, cat_smoothing=0.5)


def _case():
    domain, _trials, hist, vals = random_case(U.all_kinds_space(hp), 24, 1, 3)
    banded = [m.label for m in J.label_models(domain) if m.kind != J._L.JOINT_CAT]
    mult = dict(zip(banded, J.LOO_GRID[np.random.RandomState(1).randint(0, 16, len(banded))]))
    return domain, hist, vals, mult


def loo_loops(domain, hist, mask, mult, prior_weight, lf, a):
    """Q_set of the rows under ``mask`` with label ``lab`` at ``mult[lab]``, pair by pair."""
    labels = list(domain.params)
    names = U.joint_label_names(domain)
    cols = [labels.index(lab) for lab in names]
    infos = [U.label_info(domain.specs[lab]) for lab in names]
    comps = [U.set_components(infos, cols, hist, mask, lf, prior_weight, mult.get(lab, 1.0))[1][d]
             for d, lab in enumerate(names)]
    rows = [r for r in range(hist.tids.size) if mask[r] and all(hist.active[r, j] for j in cols)]
    n = len(rows)
    v = [float(w) for w in J.forgetting_weights(n, lf)]
    W, num = sum(v) + prior_weight, 0.0
    for i in range(n):
        x = [float(hist.vals[rows[i], j]) for j in cols]
        acc = []
        for j in list(range(n)) + [n]:
            if j == i:
                continue
            s = math.log(v[j]) if j < n else U.log_or_neg_inf(prior_weight)
            for d, info in enumerate(infos):
                s = s + U.factor(info, x[d], comps[d][j], a)
            acc.append(s)
        m = max(acc)
        lse = m if m == U.NEG_INF else m + math.log(sum(math.exp(s - m) for s in acc))
        num += v[i] * (lse - math.log(W - v[i]))
    return num / sum(v)


@pytest.mark.parametrize("label", ["c", "f"])  # (one continuous, one quantized)
def test_loo_label_numpy_is_the_double_loop(label):
    domain, hist, _vals, mult = _case()
    grid = np.asarray([0.05, 0.2, 1.5])
    Q = J.loo_label_numpy(domain, hist, mult, label, grid, **KW)
    assert Q.shape == (2, 3)
    for which, mask in enumerate(J.split_sets(hist, KW["gamma"])):
        want = [loo_loops(domain, hist, mask, dict(mult, **{label: h}), KW["prior_weight"],
                          KW["linear_forgetting"], KW["cat_smoothing"]) for h in grid]
        np.testing.assert_allclose(Q[which], want, rtol=1e-12, atol=0)


def test_equal_multipliers_are_the_scalar_curve_and_the_float():
    domain, hist, vals, mult = _case()
    ref = J.loo_numpy(domain, hist, **KW)[0]
    for b, h in enumerate(J.LOO_GRID):
        Q = J.loo_label_numpy(domain, hist, dict.fromkeys(mult, h), "g", **KW)
        np.testing.assert_allclose(Q[:, b], ref[:, b], rtol=1e-12, atol=0)
    kw = dict(prior_weight=0.7, gamma=1.2, linear_forgetting=4, cat_smoothing=0.5)
    for tree in (False, True, "chain"):
        S = J.score_numpy(domain, hist, vals, bandwidth=0.3, tree=tree, **kw)
        assert S.tobytes() == J.score_numpy(domain, hist, vals, tree=tree,
                                            bandwidth=dict.fromkeys(mult, 0.3), **kw).tobytes()
    # a label the mapping does not name takes BANDWIDTH
    assert (J.bandwidths(J.label_models(domain), 9, {}) ==
            J.bandwidths(J.label_models(domain), 9, J.BANDWIDTH)).all()


def test_choice_rules():
    grid = np.asarray([0.1, 0.2, 0.4])
    Q0 = np.asarray([[[1.0, 3.0, 3.0], [0.0, 0.0, 0.0]]])  # (the start: 0.2)
    curves = {"x": [[1.0, 2.0, 2.0], [0.0, 0.0, 0.0]],     # a tie with the current value: kept
              "y": [[5.0, 1.0, 5.0], [0.0, 0.0, np.nan]],  # the first of the largest finite
              "z": [[np.nan] * 3, [0.0] * 3]}              # nothing finite: kept
    seen = []

    def curve(mult, lab):
        seen.append((lab, dict(mult)))
        return np.asarray(curves[lab])

    mult, visited = J.loo_label_choice(grid, Q0, [[5, 5]], ["x", "y", "z"], curve, sweeps=5)
    assert mult == {"x": 0.2, "y": 0.1, "z": 0.2}
    # Gauss-Seidel: z's call already sees y's update; the second pass changes nothing and
    # ends the run (y's own curve is now 5.0 at its current value: not strictly larger)
    assert seen[2] == ("z", {"x": 0.2, "y": 0.1, "z": 0.2})
    assert [lab for lab, _ in visited] == ["x", "y", "z"] * 2 and len(seen) == 6
    assert J.loo_label_choice(grid, Q0, [[5, 5]], ["x", "y"], curve, sweeps=0)[0] == \
        {"x": 0.2, "y": 0.2}
    # the fallback: BANDWIDTH for every label, and no curve is asked for
    none = lambda mult, lab: pytest.fail("a curve was asked for")  # noqa: E731
    assert J.loo_label_choice(grid, Q0, [[1, 0]], ["x"], none) == ({"x": J.BANDWIDTH}, [])
    Q0[0, 1] = np.nan
    assert J.loo_label_choice(grid, Q0, [[5, 5]], ["x"], none) == ({"x": J.BANDWIDTH}, [])


def test_fit_never_lowers_q():
    domain, hist, _vals, _mult = _case()
    grid = J.LOO_GRID[::3]
    mult, visited = J.loo_label_fit_numpy(domain, hist, grid, sweeps=1, **KW)
    sizes = [[rows.size for rows in J.loo_sets(domain, hist, KW["gamma"])[0][1]]]
    start = J.loo_choice(grid, J.loo_numpy(domain, hist, grid, **KW), sizes)
    assert set(mult.values()) <= set(grid) and len(visited) == len(mult) == 8
    Q = [J.loo_label_numpy(domain, hist, m, "c", grid, **KW).sum(0)[list(grid).index(m["c"])]
         for m in (dict.fromkeys(mult, start), mult)]
    assert Q[1] >= Q[0] and mult != dict.fromkeys(mult, start)


@pytest.mark.parametrize("call,text", [
    (lambda d, t, p: tpe.joint_bandwidths(d, t, grid=[0.2, 0.1]), J.LOO_BAD_GRID),
    (lambda d, t, p: tpe.joint_bandwidths(d, t, sweeps=-1), "sweeps"),
    (lambda d, t, p: tpe.joint_bandwidths(d, t, sweeps=1.5), "sweeps"),
    (lambda d, t, p: tpe.joint_bandwidths(d, t, joint="chain"), J.LOO_CHAIN),
    (lambda d, t, p: tpe.joint_bandwidths(d, t, joint=False), "joint=True"),
    (lambda d, t, p: tpe.score_configs(d, t, p, joint="chain", bandwidth="loo-label"),
     J.LOO_CHAIN),
    (lambda d, t, p: tpe.score_configs(d, t, tpe.GridPool(d, {"x": [0.1, 0.2]}, joint=True),
                                       joint=True, bandwidth="loo-label"), J.LOO_GRID_POOL),
    (lambda d, t, p: tpe.score_configs(d, t, p, joint=True, bandwidth={"w": 0.2}), "not a label"),
    (lambda d, t, p: tpe.score_configs(d, t, p, joint="chain", bandwidth={"x": 0.0}), "> 0"),
    (lambda d, t, p: tpe.suggest_sampled([0], d, t, 1, joint=True, bandwidth={"x": np.inf}),
     "> 0"),
    (lambda d, t, p: tpe.Pool.sample(d, t, 1, 4, joint=True, bandwidth={"x": "a"}), "> 0"),
])
def test_argument_errors_come_before_any_engine(monkeypatch, call, text):
    monkeypatch.setattr(tpe, "engine", lambda *a, **k: pytest.fail("an engine was asked for"))
    domain, trials, _hist, _vals = random_case({"x": hp.uniform("x", 0, 1)}, 8, 1, 0)
    pool = tpe.Pool(domain, [{"x": 0.5}])
    with pytest.raises(ValueError) as err:
        call(domain, trials, pool)
    assert text in str(err.value)
