"""tpe_joint_refine on the device against ``joint.refine_numpy``.

Tolerances are the reference's own (``refine_numpy(return_info=True)``): 1e-6
per log-density, so ``J_bound`` on J, ``g_bound`` on g and ``t_bound`` on the
point reached, propagated per accepted step (joint.py).  Accepted counts are
compared exactly: a case's rows are the first of a seeded draw every decision of
which the reference alone shows to have |J(t') - J(t)| >= 100 x the bound
(``refine_util.safe_rows``), and ``_run`` asserts that of every row it sends.
"""
from functools import partial

import numpy as np
import pytest

from hyperopt_amd import Trials, fmin, hp, tpe
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from tests import joint_util as U
from tests.refine_util import KW, all_kinds_case, random_case, safe_rows

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


def _run(domain, trials, hist, vals, refine, kw=KW):
    """The kernel's climb of ``vals`` within the reference's bounds: (values, trace, J_start)."""
    ref, J0, J1, g, acc, info = J.refine_numpy(domain, hist, vals, refine, return_info=True, **kw)
    assert not (info["margin"] < 100.0).any()
    st = pool_mod._settings(kw["prior_weight"], kw["gamma"], 25, True, kw["bandwidth"],
                            kw["cat_smoothing"])
    eng, (P, L) = tpe.engine(), vals.shape
    d = tpe.Pool.from_arrays(domain, vals, np.ones(vals.shape, bool)).device(eng)
    fit = pool_mod._fit(eng, domain, hist, L, st)[0]
    tr, before = {}, d.vals[:, :P].cpu().numpy().T
    J.refine_device(fit, d.vals, d.vals.shape[1], L, P, refine, tr)
    tr = {k: v.cpu().numpy() for k, v in tr.items()}
    got, out = d.vals[:, :P].cpu().numpy().T, vals.copy()
    cont = [m for m in fit.dj.models if m.kind == J._L.JOINT_CONT]
    rest = [j for j in range(L) if j not in [m.col for m in cont]]
    assert got[:, rest].tobytes() == before[:, rest].tobytes()  # (no other column is written)
    np.testing.assert_array_equal(tr["accepted"], acc)
    np.testing.assert_array_equal(np.isnan(tr["J_start"]), np.isnan(J0))
    fin = np.isfinite(J0)
    assert (np.abs(tr["J_start"] - J0)[fin] <= info["J_bound"][fin]).all()
    # (the end points differ by t_bound: J by |g| t_bound, g by K t_bound on top)
    assert (np.abs(tr["J_end"] - J1)[fin] <=
            (info["J_bound"] + (np.abs(g) * info["t_bound"]).sum(1))[fin]).all()
    slack = np.einsum("pde,pe->pd", info["K"], info["t_bound"])
    assert (np.abs(tr["g_end"] - g)[fin] <= (info["g_bound"] + slack)[fin]).all()
    for j, m in enumerate(cont):
        out[:, m.col] = got[:, m.col]
        td, tw = J._fit(m, out[:, m.col]), J._fit(m, ref[:, m.col])
        assert (np.abs(td - tw) <= info["t_bound"][:, j] + 4 * EPS * (np.abs(tw) + 1)).all()
    assert out[acc == 0].tobytes() == vals[acc == 0].tobytes()  # (no step kept: no bit moved)
    return out, tr, J0


@pytest.mark.parametrize("refine", [0, 3])
def test_value_and_gradient_on_every_kind(refine):
    domain, trials, hist, cand = all_kinds_case(384)
    vals = safe_rows(domain, hist, cand, refine, 24)
    out, tr, J0 = _run(domain, trials, hist, vals, refine)
    nan = np.flatnonzero(np.isnan(J0))
    assert nan.size == 2 and not tr["accepted"][nan].any()  # (the two NaN rows: untouched)
    assert (refine == 0) == (not tr["accepted"].any()) == (out.tobytes() == vals.tobytes())


# T trials give (n_below + 1, n_above + 1) components under gamma = 0.25
EDGES = {0: (1, 1), 1: (2, 1), 259: (6, 255), 260: (6, 256), 261: (6, 257), 518: (7, 513)}


@pytest.mark.parametrize("refine", [1, 2, 5])
@pytest.mark.parametrize("T", sorted(EDGES))
def test_component_edges(T, refine):
    space = {"u": hp.uniform("u", -1, 2), "ln": hp.lognormal("ln", 0, 1),
             "q": hp.quniform("q", 0, 6, 2), "c": hp.choice("c", [0, 1, 2])}
    domain, trials, hist, cand = random_case(space, T, 128, 100 + T)
    sizes = tuple(J.set_rows(hist, m, list(range(4))).size + 1 for m in J.split_sets(hist, 0.25))
    assert sizes == EDGES[T]
    kw = dict(KW, gamma=0.25)
    tr = _run(domain, trials, hist, safe_rows(domain, hist, cand, refine, 24, kw), refine, kw)[1]
    assert (T == 0) == (not tr["accepted"].any())  # (both sets empty: J is 0 everywhere)


@pytest.mark.parametrize("Dc", [1, J._L.REFINE_MAX_CONT])
def test_continuous_label_count_edges(Dc):
    space = {"x%02d" % i: hp.normal("x%02d" % i, 0, 1) for i in range(Dc)}
    space["c"] = hp.choice("c", [0, 1])
    domain, trials, hist, cand = random_case(space, 60, 64, 7)
    # (far from every trial the two priors cancel and J is flat: start near the best two)
    xs = [list(domain.params).index(lab) for lab in sorted(space) if lab != "c"]
    near = np.asarray(hist.vals)[np.argsort(hist.losses)[:2]][np.arange(64) % 2]
    cand[:, xs] = near[:, xs] + 0.4 * np.random.RandomState(1).randn(64, Dc)
    # (two steps: a third is at the peak and has no margin)
    tr = _run(domain, trials, hist, safe_rows(domain, hist, cand, 2, 16), 2)[1]
    assert tr["g_end"].shape == (16, Dc) and tr["accepted"].all()


def test_clamping():
    """At ``u``'s lower bound g points outward: it stays; the log label moves, positive."""
    space = {"u": hp.uniform("u", 0, 1), "lg": hp.loguniform("lg", -3, 0)}
    domain, trials, hist, cand = random_case(space, 120, 96, 3, loss=lambda c: c["u"])
    iu, ig = list(domain.params).index("u"), list(domain.params).index("lg")
    cand[:, iu] = 0.0
    vals = safe_rows(domain, hist, cand, 4, 16)
    out, tr, _J0 = _run(domain, trials, hist, vals, 4)
    first = J.refine_numpy(domain, hist, vals, 0, **KW)[3]
    assert (first[:, sorted([iu, ig]).index(iu)] < 0).all() and tr["accepted"].all()
    assert out[:, iu].tobytes() == vals[:, iu].tobytes()
    assert (out[:, ig] > 0).all() and (out[:, ig] != vals[:, ig]).all()


def test_the_point_of_it():
    """Good trials on the ridge y = x, rows on a coarse lattice that misses it."""
    space = {"x": hp.uniform("x", 0, 1), "y": hp.uniform("y", 0, 1)}
    domain, trials, hist, _ = random_case(space, 200, 0, 11, loss=lambda c: abs(c["x"] - c["y"]))
    a = 0.2 * np.arange(5)
    vals = np.stack([np.repeat(a + 0.05, 5), np.tile(a + 0.17, 5)], 1)
    _ref, J0, J1, g, _acc, info = J.refine_numpy(domain, hist, vals, 8, return_info=True, **KW)
    w = int(np.argmax(J1))
    assert J1[w] - J0.max() > 100 * info["J_bound"][w]
    out, Jb, Ja, acc, _g = tpe.refine_configs(domain, trials, vals, 8, return_trace=True, **KW)
    assert (Ja >= Jb).all() and acc.all() and int(np.argmax(Ja)) == w
    assert abs(Ja[w] - J1[w]) <= info["J_bound"][w] + (np.abs(g[w]) * info["t_bound"][w]).sum()
    # k rows give k results that do not depend on one another
    part = tpe.refine_configs(domain, trials, vals[3::4], 8, **KW)
    assert part.tobytes() == out[3::4].tobytes()
    assert tpe.refine_configs(domain, trials, vals, 0, **KW).tobytes() == vals.tobytes()


def test_public_path():
    domain, trials, _hist, _vals = all_kinds_case()
    moving = [m.label for m in J.label_models(domain) if m.kind == J._L.JOINT_CONT]
    kw = dict(KW, n_EI_candidates=512, joint=True, draw="joint", verbose=False)

    def docs(seed=9, **more):
        got = tpe.suggest_sampled(range(200, 204), domain, trials, seed, **dict(kw, **more))
        return [d["misc"]["vals"] for d in got]

    plain, refined = docs(), docs(refine=8)
    assert len(refined) == 4 and docs(refine=0) == plain and docs(refine=8) == refined
    for a, b in zip(plain, refined):
        assert {k: v for k, v in a.items() if k not in moving} == \
            {k: v for k, v in b.items() if k not in moving}
        assert all(a[k] != b[k] for k in moving)
    assert docs(seed=10, refine=8) != refined
    liar = docs(refine=8, batch="liar")
    assert len(liar) == 4 and liar[0] == refined[0]
    run = Trials()
    fmin(lambda c: (c["c"] - 5.0) ** 2 + abs(c["g"]), U.all_kinds_space(hp),
         algo=partial(tpe.suggest_sampled, n_EI_candidates=128, joint=True, draw="joint",
                      refine=4, verbose=False),
         max_evals=30, max_queue_len=2, trials=run, rstate=np.random.RandomState(0),
         show_progressbar=False)
    assert len(run) == 30
