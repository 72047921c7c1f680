"""The leave-one-out bandwidth criterion on the host (joint.py, "Bandwidth"):
``loo_numpy`` against a plain double loop, the rules of the choice, and the
argument errors, each raised before any engine exists."""
import math

import numpy as np
import pytest

from hyperopt_amd import hp, tpe
from hyperopt_amd import joint as J
from tests import joint_util as U
from tests.refine_util import random_case

KW = dict(prior_weight=0.7, gamma=1.2, linear_forgetting=4, cat_smoothing=0.5)


def loo_loops(domain, hist, mask, h, prior_weight, lf, a):
    """Q_set of the rows under ``mask`` at multiplier h, pair by pair."""
    labels = list(domain.params)
    names = U.joint_label_names(domain)
    cols = [labels.index(lab) for lab in names]
    infos = [U.label_info(domain.specs[lab]) for lab in names]
    _logw, comps, n = U.set_components(infos, cols, hist, mask, lf, prior_weight, h)
    rows = [r for r in range(hist.tids.size) if mask[r] and all(hist.active[r, j] for j in cols)]
    if n < 2:
        return 0.0
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


def test_loo_numpy_is_the_double_loop():
    domain, _trials, hist, _vals = random_case(U.all_kinds_space(hp), 24, 1, 3)
    grid = np.asarray([0.05, 0.2, 1.5])
    Q = J.loo_numpy(domain, hist, grid, **KW)
    assert Q.shape == (1, 2, 3)
    sizes = [rows.size for rows in J.loo_sets(domain, hist, KW["gamma"])[0][1]]
    assert sizes[0] == 6 and sizes[1] > KW["linear_forgetting"]  # (the ramp is not flat)
    for which, mask in enumerate(J.split_sets(hist, KW["gamma"])):
        want = [loo_loops(domain, hist, mask, h, KW["prior_weight"], KW["linear_forgetting"],
                          KW["cat_smoothing"]) for h in grid]
        np.testing.assert_allclose(Q[0, which], want, rtol=1e-12, atol=0)


def test_choice_rules():
    grid = np.asarray([0.1, 0.2, 0.4])
    Q = np.asarray([[[1.0, 3.0, 3.0], [0.0, 0.0, 0.0]]])
    assert J.loo_choice(grid, Q, [[5, 1]]) == 0.2  # (the first of the largest)
    assert J.loo_choice(grid, Q, [[1, 0]]) == J.BANDWIDTH  # (no set with n >= 2)
    Q[0, 1] = [-np.inf, np.nan, -np.inf]
    assert J.loo_choice(grid, Q, [[5, 5]]) == J.BANDWIDTH  # (no finite Q)
    Q[0, 1] = [0.0, np.nan, -1.0]
    assert J.loo_choice(grid, Q, [[5, 5]]) == 0.4  # (the largest finite one)
    # a set with n < 2 is 0 for every h; the default grid holds BANDWIDTH
    domain, _trials, hist, _vals = random_case({"x": hp.uniform("x", 0, 1)}, 2, 1, 0)
    assert not J.loo_numpy(domain, hist, gamma=0.25)[0, 0].any()
    assert J.LOO_GRID.size == J._L.LOO_MAX_GRID and J.LOO_GRID[6] == J.BANDWIDTH


@pytest.mark.parametrize("call,text", [
    (lambda d, t, p: tpe.joint_bandwidth(d, t, grid=[]), J.LOO_BAD_GRID),
    (lambda d, t, p: tpe.joint_bandwidth(d, t, grid=[0.2, 0.1]), J.LOO_BAD_GRID),
    (lambda d, t, p: tpe.joint_bandwidth(d, t, grid=[0.0, 0.1]), J.LOO_BAD_GRID),
    (lambda d, t, p: tpe.joint_bandwidth(d, t, grid=np.linspace(0.1, 1, 17)), J.LOO_BAD_GRID),
    (lambda d, t, p: tpe.joint_bandwidth(d, t, joint="chain"), J.LOO_CHAIN),
    (lambda d, t, p: tpe.score_configs(d, t, p, joint="chain", bandwidth="loo"), J.LOO_CHAIN),
    (lambda d, t, p: tpe.score_configs(d, t, tpe.GridPool(d, {"x": [0.1, 0.2]}, joint=True),
                                       joint=True, bandwidth="loo"), J.LOO_GRID_POOL),
    (lambda d, t, p: tpe.score_configs(d, t, p, joint=True, bandwidth="cv"), "or 'loo'"),
])
def test_argument_errors_come_before_any_engine(monkeypatch, call, text):
    monkeypatch.setattr(tpe, "engine", lambda *a, **k: pytest.fail("an engine was asked for"))
    domain, trials, _hist, _vals = random_case({"x": hp.uniform("x", 0, 1)}, 8, 1, 0)
    pool = tpe.Pool(domain, [{"x": 0.5}])
    with pytest.raises(ValueError) as err:
        call(domain, trials, pool)
    assert text in str(err.value)
