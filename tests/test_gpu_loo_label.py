"""tpe_joint_loo_label on the device against ``joint.loo_label_numpy`` (joint.py,
"Bandwidth per label").

The tolerance is the project's 1e-6 relative per log-density (``REFINE_TOL``)
times max(1, |Q_ref|) per curve value; -inf and NaN must sit where the
reference's do."""
import functools

import numpy as np
import pytest

from hyperopt_amd import Domain, hp, tpe
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from tests import joint_tree_util as TU
from tests import joint_util as U
from tests.refine_util import random_case
from tests.test_gpu_loo import KW, _cluster, _edge_case, _flat, _tol
from tests.test_gpu_refine import EDGES

pytestmark = pytest.mark.gpu
G = J.LOO_GRID


def _check(domain, hist, mult, label, grid, ref, tree=False, kw=KW):
    eng = tpe.engine()
    curve = J.loo_label_curves(eng, domain, hist, pool_mod._seen_rows(eng, hist), kw["gamma"],
                               len(domain.params), grid, kw["prior_weight"],
                               kw["linear_forgetting"], kw["cat_smoothing"], tree)
    got = curve(mult, label)
    print("device", got, "reference", ref, sep="\n")
    assert got.shape == ref.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_array_equal(got == -np.inf, ref == -np.inf)
    fin = np.isfinite(ref)
    assert (np.abs(got - ref)[fin] <= _tol(ref)[fin]).all()
    return got


@pytest.mark.parametrize("label", list("cdefghij"))  # (every label with a bandwidth)
def test_every_kind(label):
    domain, _trials, hist, _vals = random_case(U.all_kinds_space(hp), 60, 1, 5)
    kw = dict(KW, gamma=1.0, linear_forgetting=20)  # (8 below; a ramp over the 51 above)
    mult = dict(zip("cdefghij", G[np.random.RandomState(7).randint(0, 16, 8)]))
    _check(domain, hist, mult, label, None, J.loo_label_numpy(domain, hist, mult, label, **kw),
           kw=kw)


# the other labels at unequal multipliers: one shared scale cannot pass
EDGE_MULT = {"u": G[3], "ln": G[10], "q": G[5]}


@functools.lru_cache(None)
def _edge_ref(T, label):
    domain, hist, _ref = _edge_case(T)
    return J.loo_label_numpy(domain, hist, EDGE_MULT, label, **KW)


@pytest.mark.parametrize("label", ["u", "q"])
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("T", sorted(EDGES))
def test_chunk_and_block_edges(T, B, label):
    domain, hist, _ref = _edge_case(T)
    pick = np.arange(16)[::16 // B][:B]  # (the smallest multiplier is always among them)
    got = _check(domain, hist, EDGE_MULT, label, G[pick], _edge_ref(T, label)[:, pick])
    assert (T < 259) == (not got.any())  # (no set with two rows: 0 everywhere)


@pytest.mark.parametrize("case", ["isolated", "twins"])
def test_self_exclusion_is_by_index(case):
    pts = _cluster(40, 2, 0.05)
    pts[17] = (0.97, 3.0) if case == "isolated" else pts[3]
    domain, _trials, hist = _flat(pts, 4)
    grid, mult = G[:1], {"x": G[0], "y": G[4]}  # (the smallest grid value for d = x)
    ref = J.loo_label_numpy(domain, hist, mult, "x", grid, **KW)
    if case == "isolated":  # the self term, left in, would move Q by far more than the tolerance
        (models, sets), lf, pw = J.loo_sets(domain, hist, KW["gamma"])[0], 25, KW["prior_weight"]
        for which, rows in enumerate(sets):
            v = J.forgetting_weights(rows.size, lf)
            x = np.asarray(hist.vals)[rows][:, [m.col for m in models]]
            L = J._set_log_l(models, hist, rows, x, lf, pw, mult, KW["cat_smoothing"])
            W = v.sum() + pw
            with_self = (v * (L + np.log(W) - np.log(W - v))).sum() / v.sum()
            assert abs(with_self - ref[which, 0]) >= 100 * _tol(ref[which, 0])
    _check(domain, hist, mult, "x", grid, ref)


def test_groups():
    domain, trials = TU.branch_diagonal_case()
    hist = tpe.collect_history(trials, list(domain.params))
    kw = dict(KW, gamma=TU.GAMMA_DIAGONAL)
    ref = J.loo_label_numpy(domain, hist, {"c": G[2]}, "c", tree=True, **kw)
    assert ref.any()
    _check(domain, hist, {"c": G[2]}, "c", None, ref, tree=True, kw=kw)


@pytest.mark.parametrize("seed", [0, 3])
def test_public_path(seed):
    # the loss is a function of x alone; x is clustered, y is N(0, 1) whatever x is
    rng = np.random.RandomState(seed)
    x, y = np.clip(0.5 + 0.03 * rng.randn(120), 0.01, 0.99), rng.randn(120)
    domain = Domain(lambda c: 0, {"x": hp.uniform("x", 0, 1), "y": hp.normal("y", 0, 1)})
    trials = U.make_trials(domain, [{"x": float(a), "y": float(b)} for a, b in zip(x, y)],
                           np.abs(x - 0.5))
    hist = tpe.collect_history(trials, list(domain.params))
    kw = dict(prior_weight=KW["prior_weight"], gamma=KW["gamma"], cat_smoothing=0.5)
    Q0 = J.loo_numpy(domain, hist, **kw)
    h = J.loo_choice(G, Q0, [[r.size for r in J.loo_sets(domain, hist, kw["gamma"])[0][1]]])
    want, visited = J.loo_label_fit_numpy(domain, hist, **kw)
    assert want["x"] < h < want["y"]
    with np.errstate(invalid="ignore"):
        for Q in [Q0.sum((0, 1))] + [c.sum(0) for _lab, c in visited]:  # (every decision taken)
            Q = np.sort(Q[np.isfinite(Q)])[::-1]
            assert Q[0] - Q[1] >= 100 * _tol(Q[0])  # (no choice is a coin toss)
    got, grid, curves = tpe.joint_bandwidths(domain, trials, return_curves=True, **kw)
    assert got == want == tpe.joint_bandwidths(domain, trials, **kw)
    assert [lab for lab, _c in curves] == [lab for lab, _c in visited] and grid.size == 16
    pool = tpe.Pool.from_arrays(domain, _cluster(64, 1, 1.0), np.ones((64, 2), bool))
    score = functools.partial(tpe.score_configs, domain, trials, pool, joint=True, **kw)
    assert score(bandwidth="loo-label").tobytes() == score(bandwidth=want).tobytes()
    assert score(bandwidth={"x": h, "y": h}).tobytes() == score(bandwidth=h).tobytes()
    assert score(bandwidth=want).tobytes() != score(bandwidth=h).tobytes()
