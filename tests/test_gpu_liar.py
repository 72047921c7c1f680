"""The liar batch on the GPU through the public API (csrc/tpe_joint_lie.hip
under tpe.pick_batch, suggest_from_pool and suggest_sampled with
``batch="liar"``), against the scalar restatement in tests/liar_util.py.

Tolerance: the project's fp64 log-density tolerance, 1e-6 relative per
log-density (test_gpu_parity.py, test_gpu_joint.py), counted once per
log-density that enters S_k = (log L_below - A_0) - (U_k - U_0):
|S_k - ref| <= 1e-6 (|log L_below| + |A_0| + |U_0| + |U_k|).  Picks are
compared exactly, after the reference alone has shown that every pick beats
its runner-up by at least 100 times that bound.
"""
from functools import partial

import numpy as np
import pytest

from hyperopt_amd import Domain, Trials, fmin, hp, tpe
from hyperopt_amd import pool as pool_mod
from tests import joint_util as U
from tests import liar_util as LU
from tests.test_gpu_joint import KW, P_ROWS, _all_kinds

pytestmark = pytest.mark.gpu

K = 6
_SHARED = {}


def _ref_kw(kw):
    return dict(prior_weight=kw["prior_weight"], gamma=kw["gamma"], lf=kw["linear_forgetting"],
                bandwidth=kw["bandwidth"], cat_smoothing=kw["cat_smoothing"])


def _fresh(domain, pool):
    return tpe.Pool.from_arrays(domain, pool.vals, pool.active)


def _bound(ref_b, ref_a, ref):
    return 1e-6 * (np.abs(ref_b) + np.abs(ref_a) + np.abs(ref["U_0"]) + np.abs(ref["U_k"]))


def _check_margins(ref, bound, fin):
    """From the reference alone: every pick at a score that is not NaN beats
    its runner-up (exact twins excepted) by >= 100 x the bound."""
    gaps = ref["gaps"][~np.isnan(ref["gaps"])]
    print("reference gaps", gaps, "bound %.3g" % bound[fin].max())
    assert gaps.size and (gaps >= 100.0 * bound[fin].max()).all()


# -- 1. values -------------------------------------------------------------------
def test_values_and_picks_match_scalar_restatement():
    domain, trials, pool, (ref_j, ref_b, ref_a, _nb, _na) = _all_kinds()
    ref = LU.liar_reference(domain, trials, pool.vals, ref_j, ref_a, K, **_ref_kw(KW))
    fin = ~np.isnan(ref_j)
    assert np.flatnonzero(~fin).tolist() == [5, 299]
    bound = _bound(ref_b, ref_a, ref)
    assert ref["rows"][:2] == [5, 299] and len(ref["rows"]) == K
    assert np.isnan(ref["gaps"][:2]).all() and not np.isnan(ref["gaps"][2:]).any()
    _check_margins(ref, bound, fin)
    fresh = _fresh(domain, pool)
    rows, at, S_k = tpe.pick_batch(domain, trials, fresh, K, return_trace=True, **KW)
    assert rows.dtype == np.int64 and rows.tolist() == ref["rows"]  # NaN rows first, in row order
    assert not fresh.taken.any() and not fresh.row_of               # nothing is marked
    np.testing.assert_array_equal(np.isnan(S_k), ~fin)
    err = np.abs(S_k[fin] - ref["S_k"][fin])
    print("max |S_k - ref| = %.3g (bound %.3g)" % (err.max(), bound[fin].max()))
    assert (err <= bound[fin]).all()
    assert np.isnan(at[:2]).all()
    assert (np.abs(at[2:] - ref["S_at_pick"][2:]) <= bound[rows[2:]]).all()
    # S_0 keeps the bits it has without ``batch``: nothing was picked at k = 0
    S0 = tpe.score_configs(domain, trials, fresh, joint=True, **KW)
    none, at0, S_0 = tpe.pick_batch(domain, trials, fresh, 0, return_trace=True, **KW)
    assert none.size == 0 and at0.size == 0
    assert (S_0.view(np.uint64) == S0.view(np.uint64)).all()
    assert at[2] == S0[rows[2]]  # the first pick of a real score: at S_0, bit for bit
    assert tpe.pick_batch(domain, trials, fresh, K, **KW).tolist() == ref["rows"]


# -- 2. equivalence --------------------------------------------------------------
def test_first_document_is_the_one_without_batch():
    domain, trials, pool, _ = _all_kinds()

    def docs(k, **kw):
        p = _fresh(domain, pool)
        p.mark_taken([5, 299])  # (the NaN rows: let real scores decide)
        ids = list(range(900, 900 + k))
        out = tpe.suggest_from_pool(ids, domain, trials, 0, pool=p, joint=True, verbose=False,
                                    **dict(KW, **kw))
        assert [p.taken[p.row_of[i]] for i in ids] == [1] * k
        return [d["misc"]["vals"] for d in out], [p.row_of[i] for i in ids]

    plain1, liar1 = docs(1), docs(1, batch="liar")
    assert plain1 == liar1
    plain4, liar4 = docs(4), docs(4, batch="liar", lie_weight=2.0)
    assert len(liar4[0]) == 4 and len(set(liar4[1])) == 4
    assert plain4[0][0] == liar4[0][0] == plain1[0][0]
    assert plain4[1][0] == liar4[1][0] == plain1[1][0]


# -- 3. diversity ----------------------------------------------------------------
# (gamma 1.5: the below set is the ceil(1.5 sqrt(40)) = 10 good trials)
DIV_KW = dict(prior_weight=1.0, gamma=1.5, linear_forgetting=25, bandwidth=0.2, cat_smoothing=1.0)


def _plain_top(S0, k):
    """The first k rows of one score vector, and each one's gap to the next."""
    S, gone, rows, gaps = [float(s) for s in S0], [False] * len(S0), [], []
    for _ in range(k):
        p = LU.first_row(S, gone)
        gone[p] = True
        rows.append(p)
        gaps.append(S[p] - S[LU.first_row(S, gone)])
    return dict(rows=rows, gaps=np.asarray(gaps))


def _diversity_case():
    """A bounded two-label space whose good trials sit at one point, and a
    32 x 32 lattice pool around it (the point is off the lattice and off its
    axes of symmetry: no two rows tie but for rounding)."""
    if "div" not in _SHARED:
        domain = Domain(lambda x: 0, {"x": hp.uniform("x", 0, 1), "y": hp.uniform("y", 0, 1)})
        rng = np.random.RandomState(4)
        good = [{"x": 0.5037 + 1e-3 * rng.randn(), "y": 0.4971 + 1e-3 * rng.randn()}
                for _ in range(10)]
        bad = [{"x": float(rng.uniform()), "y": float(rng.uniform())} for _ in range(30)]
        trials = U.make_trials(domain, good + bad, [0.01 * i for i in range(10)] +
                               [1.0 + 0.01 * i for i in range(30)])
        grid = 0.5 + 0.03 * (np.arange(32) - 15.5)
        rows = [{"x": float(a), "y": float(b)} for a in grid for b in grid]
        pool = tpe.Pool(domain, rows)
        ref_j, ref_b, ref_a, nb, na = U.joint_reference(domain, trials, pool.vals,
                                                        **_ref_kw(DIV_KW))
        assert (nb, na) == (10, 30)
        ref = LU.liar_reference(domain, trials, pool.vals, ref_j, ref_a, 8, **_ref_kw(DIV_KW))
        plain = _plain_top(ref_j, 8)
        _SHARED["div"] = (domain, trials, pool, (ref_j, ref_b, ref_a), ref, plain)
    return _SHARED["div"]


def _spread(pool, rows):
    """Mean pairwise distance of the rows' configurations."""
    v = pool.vals[rows]
    d = np.sqrt(((v[:, None, :] - v[None, :, :]) ** 2).sum(-1))
    return d[np.triu_indices(len(rows), 1)].mean()


def test_liar_batch_spreads_where_the_top_k_crowds():
    domain, trials, pool, (ref_j, ref_b, ref_a), ref, plain = _diversity_case()
    # from the reference first: the liar's picks are not the plain top 8, and lie wider
    assert len(ref["rows"]) == 8 and ref["rows"][0] == plain["rows"][0]
    assert set(ref["rows"]) != set(plain["rows"])
    print("spread: top-8 %.4f, liar %.4f" % (_spread(pool, plain["rows"]),
                                               _spread(pool, ref["rows"])))
    assert _spread(pool, ref["rows"]) > 2.0 * _spread(pool, plain["rows"])
    fin = np.ones(len(pool), bool)
    _check_margins(ref, _bound(ref_b, ref_a, ref), fin)
    _check_margins(plain, _bound(ref_b, ref_a, ref), fin)
    # the device returns the reference's picks, with and without the lie
    assert tpe.pick_batch(domain, trials, pool, 8, **DIV_KW).tolist() == ref["rows"]
    ids = list(range(500, 508))
    tpe.suggest_from_pool(ids, domain, trials, 0, pool=pool, joint=True, batch="liar",
                          verbose=False, **DIV_KW)
    assert [pool.row_of[i] for i in ids] == ref["rows"]
    pool.release(ref["rows"])
    tpe.suggest_from_pool(ids, domain, trials, 0, pool=pool, joint=True, verbose=False, **DIV_KW)
    assert [pool.row_of[i] for i in ids] == plain["rows"]
    pool.release(plain["rows"])


# -- 4. a sampled pool -----------------------------------------------------------
def _quantized_case():
    domain = Domain(lambda x: 0, {"q": hp.quniform("q", 0, 10, 1), "r": hp.quniform("r", 0, 5, 1),
                                  "c": hp.choice("c", [0, 1, 2])})
    rng = np.random.RandomState(8)
    configs = [{"q": float(rng.randint(0, 11)), "r": float(rng.randint(0, 6)),
                "c": int(rng.randint(0, 3))} for _ in range(30)]
    losses = [abs(c["q"] - 6.0) + abs(c["r"] - 2.0) + 0.01 * i for i, c in enumerate(configs)]
    return domain, U.make_trials(domain, configs, losses), configs


def test_suggest_sampled_joint_draw_liar_distinct():
    domain, trials, configs = _quantized_case()
    ids = list(range(300, 306))
    kw = dict(n_EI_candidates=512, joint=True, draw="joint", batch="liar", distinct=True,
              verbose=False)
    docs = tpe.suggest_sampled(ids, domain, trials, 21, **kw)
    assert len(docs) == 6
    got = [tuple(d["misc"]["vals"][lab][0] for lab in ("q", "r", "c")) for d in docs]
    assert len(set(got)) == 6                                      # pairwise distinct
    seen = {(c["q"], c["r"], c["c"]) for c in configs}
    assert not set(got) & seen                                     # none is in trials
    again = tpe.suggest_sampled(ids, domain, trials, 21, **kw)
    assert [d["misc"] for d in again] == [d["misc"] for d in docs]  # a function of the seed
    # the first document is the plain call's; draw="factorised" takes the batch too
    plain = tpe.suggest_sampled(ids, domain, trials, 21, **dict(kw, batch=None))
    assert plain[0]["misc"]["vals"] == docs[0]["misc"]["vals"]
    other = tpe.suggest_sampled(ids, domain, trials, 21, **dict(kw, draw="factorised"))
    base = tpe.suggest_sampled(ids, domain, trials, 21, **dict(kw, draw="factorised", batch=None))
    assert len(other) == 6 and other[0]["misc"]["vals"] == base[0]["misc"]["vals"]


# -- 5. fmin ---------------------------------------------------------------------
def test_fmin_with_a_queue_of_four():
    space = {"x": hp.uniform("x", -2, 2), "q": hp.quniform("q", 0, 8, 1),
             "c": hp.choice("c", [0, 1, 2])}
    trials = Trials()
    algo = partial(tpe.suggest_sampled, n_EI_candidates=256, joint=True, draw="joint",
                   batch="liar", verbose=False)
    fmin(lambda cfg: (cfg["x"] - 0.5) ** 2 + abs(cfg["q"] - 3.0) + float(cfg["c"] != 1), space,
         algo=algo, max_evals=60, max_queue_len=4, trials=trials,
         rstate=np.random.RandomState(0), show_progressbar=False)
    assert len(trials) == 60  # 20 startup evaluations, then 40 in batches of four


# -- 6. the startup phase --------------------------------------------------------
def test_startup_phase_is_unchanged_by_batch():
    domain, trials, pool, _ = _all_kinds()
    ids = [40, 41, 42]
    rows = []
    for kw in (dict(), dict(batch="liar")):
        p = _fresh(domain, pool)
        tpe.suggest_from_pool(ids, domain, trials, 7, pool=p, joint=True, n_startup_jobs=10 ** 6,
                              verbose=False, **dict(KW, **kw))
        rows.append([p.row_of[i] for i in ids])
    assert rows[0] == rows[1] and len(set(rows[0])) == 3
    assert rows[0] == pool_mod.startup_rows(_fresh(domain, pool), 7, 3).tolist()
    start = dict(n_EI_candidates=64, n_startup_jobs=10 ** 6, joint=True, draw="joint",
                 verbose=False)
    d1 = tpe.suggest_sampled(ids, domain, trials, 9, batch="liar", **start)
    d2 = tpe.suggest_sampled(ids, domain, trials, 9, **start)
    assert [d["misc"]["vals"] for d in d1] == [d["misc"]["vals"] for d in d2]
    assert P_ROWS == len(pool)
