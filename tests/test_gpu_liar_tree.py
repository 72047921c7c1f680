"""csrc/tpe_joint_lie_tree.hip on the GPU: the picks on synthetic S_0 / A,
tpe_rows_scatter, ``score_tree_device(above=)`` and the public path.

S_0, A and log W_g are inputs, so S_k carries the error of the U_gk alone: |S_k -
ref| <= 1e-6 sum over the row's live groups of (|U_g0| + |U_gk|), the project's
fp64 log-density tolerance, against tests/test_liar_tree_host.py's restatement.
Picks must be the restatement's: the free rows' S_0 lie 0.5 apart, and the
restatement alone shows every pick >= 100 bounds ahead of its runner-up (the
seeds of ``_case``, every case below).
"""
import functools
import math

import numpy as np
import pytest

from hyperopt_amd import Domain, Trials, fmin, hp, rand, tpe
from hyperopt_amd import _lib as L
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from tests import joint_util as U
from tests.test_liar_tree_host import group_sets, tolerance, tree_lie_picks

pytestmark = pytest.mark.gpu

SMOOTHING, BW, LIE = 0.5, 0.25, 0.8
SPACES = {
    # one label of each factor kind, as test_gpu_liar_stages.py's "kinds"
    "flat": lambda: {"u": hp.loguniform("u", -2, 1), "v": hp.qlognormal("v", 0, 1, 0.5),
                     "w": hp.pchoice("w", [(0.0, 0), (0.3, 1), (0.7, 2)])},
    # no label has a bandwidth: the tree call takes no sigmas at all
    "cats": lambda: {"a": hp.pchoice("a", [(0.2, 0), (0.3, 1), (0.5, 2)]), "b": hp.randint("b", 4)},
    # root, two branches mixed inside every wave, two nested groups, a branch never taken
    "tree": lambda: {"r": hp.loguniform("r", -2, 1), "s": hp.choice("s", [
        {"q": hp.qlognormal("q", 0, 1, 0.5), "n": hp.normal("n", 0, 1)},
        {"w": hp.pchoice("w", [(0.0, 0), (0.3, 1), (0.7, 2)]),
         "t": hp.choice("t", [{"z": hp.quniform("z", 0, 8, 2)}, {"zz": hp.randint("zz", 3)}])},
        {"lone": hp.uniform("lone", 0, 1)}])},
}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(None)
def _case(shape, P):
    """40 trials and P rows of the space; 24 free rows, the first and the last
    among them; past P = 8 one free score is NaN and two places of A are -inf."""
    rng = np.random.RandomState(P)
    domain = Domain(lambda x: 0, SPACES[shape]())
    cfgs = [c for c in (rand.sample_config(domain, rng) for _ in range(3 * P + 200))
            if c.get("s") != 2]
    trials = U.make_trials(domain, cfgs[:40], rng.uniform(size=40))
    pool = tpe.Pool(domain, cfgs[40:40 + P])
    sets = group_sets(domain, trials, bandwidth=BW)
    free = np.unique(np.concatenate([[0, P - 1], rng.permutation(P)[:22]]))
    S0 = rng.normal(0, 1, P)
    S0[free] = 0.5 * rng.permutation(free.size) + rng.uniform(0, 0.1, free.size)
    A = rng.uniform(-6, 2, (P, len(sets)))
    gone = np.ones(P, np.uint8)
    gone[free] = 0
    if P > 8:
        S0[free[3]] = np.nan
        A[free[5], 0], A[free[7], len(sets) - 2] = -np.inf, -np.inf
    live = np.stack([pool.active[:, s[1][0]] for s in sets], 1).astype(bool)
    assert shape != "tree" or P < 8 or (live[:, 1:5].any(0).all() and not live[:, 5].any())
    return domain, trials, pool, sets, live, S0, A, gone


def _device(shape, P, k, rows=None, flat=False):
    import torch as t
    domain, trials, pool, _sets, _live, S0, A, gone = _case(shape, P)
    sel = np.arange(P) if rows is None else rows
    eng = tpe.engine()
    d = tpe.Pool.from_arrays(domain, pool.vals[sel], pool.active[sel]).device(eng)
    fits = pool_mod._fit(eng, domain, tpe.collect_history(trials, pool.labels), len(pool.labels),
                         pool_mod._settings(1.0, 0.25, 25, "tree", BW, SMOOTHING))
    up = lambda a: t.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    odd = (np.arange(P) % 2).astype(np.uint8)
    args = (d.vals.shape[1], d.vals.shape[0], sel.size, up(S0[sel]))
    tail = (up((gone * odd)[sel]), up((gone * (1 - odd))[sel]), k, LIE, True)
    if flat:
        return J.liar_device(fits[0], d.vals, *args, up(A[sel, 0]), *tail)
    return J.liar_tree_device(fits, d.vals, d.active, *args, up(A[sel].T), *tail)


@pytest.mark.parametrize("shape", ["flat", "tree"])
@pytest.mark.parametrize("P", [1, 256, 257, 600])
def test_picks_and_scores_match_scalar_restatement(shape, P):
    _domain, _trials, pool, sets, live, S0, A, gone = _case(shape, P)
    for k in (1, 3, P + 2):
        ref = tree_lie_picks(sets, pool.vals, live, S0, A, math.log(LIE), SMOOTHING, k, gone)
        margin = ref["margin"][~np.isnan(ref["margin"])]
        assert (margin >= 100.0).all()  # (the restatement's own: the inputs' property)
        rows, at, S_k = _device(shape, P, k)
        assert rows.tolist() == ref["rows"] and len(rows) == min(k, int((gone == 0).sum()))
        bound = tolerance(ref, 1e-6)
        for got, want, b in ((S_k, ref["S_k"], bound), (at, ref["S_at_pick"], bound[rows])):
            np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
            np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
            ok = np.isfinite(want)
            assert (np.abs(got[ok] - want[ok]) <= b[ok]).all(), np.abs(got[ok] - want[ok]).max()
        still = (_bits(np.nan_to_num(ref["U_k"])) == _bits(np.nan_to_num(ref["U_0"]))).all(1)
        still &= ~np.isnan(S0)
        assert (_bits(S_k[still]) == _bits(S0[still])).all()  # untouched groups subtract 0.0
        assert (_bits(at[:1]) == _bits(S0[rows[:1]])).all()


@pytest.mark.parametrize("shape,P,k", [("flat", 1, 1), ("flat", 257, 3), ("flat", 600, 602),
                                       ("cats", 257, 602)])
def test_one_group_has_the_bits_of_the_flat_call(shape, P, k):
    tree, flat = _device(shape, P, k), _device(shape, P, k, flat=True)
    assert tree[0].tolist() == flat[0].tolist() and len(tree[0]) in (k, 23, 24)
    assert (_bits(tree[1]) == _bits(flat[1])).all() and (_bits(tree[2]) == _bits(flat[2])).all()
    assert P == 1 or not (_bits(tree[2]) == _bits(_case(shape, P)[5])).all()


def test_bits_do_not_depend_on_the_pool_shape():
    rows, at, S_k = _device("tree", 600, 6)
    rest = np.setdiff1d(np.arange(600), rows)
    sub = np.sort(np.concatenate([rows, np.random.RandomState(9).permutation(rest)[:251]]))
    rows2, at2, S_k2 = _device("tree", 600, 6, rows=sub)
    assert sub.size == 257 and sub[rows2].tolist() == rows.tolist()
    assert (_bits(S_k2) == _bits(S_k[sub])).all() and (_bits(at2) == _bits(at)).all()


@pytest.mark.parametrize("n,begin,win", [(0, 0, 8), (1, 0, 8), (256, 0, 256), (257, 0, 512),
                                         (257, 256, 256), (300, 0, 257)])
def test_rows_scatter_matches_numpy(n, begin, win):
    import torch as t
    eng, lib, ld = tpe.engine(), L.load(), 700
    rng = np.random.RandomState(n)
    rows = np.full(ld, 3, np.int64)  # (past the count: a valid row nobody may write)
    rows[:n] = np.sort(rng.permutation(np.arange(4, ld))[:n])
    if n > 2:
        rows[1], rows[n - 1] = -1, ld  # outside [0, ld): skipped
    src = rng.normal(size=win)
    want = np.full(ld + 8, -7.5)
    for p in [p for p in range(begin, min(begin + win, n)) if 0 <= rows[p] < ld]:
        want[rows[p]] = src[p - begin]
    d_rows, d_src, dst = (t.from_numpy(a).to(eng.device) for a in (rows, src, np.full(ld + 8, -7.5)))
    count = t.tensor([n], dtype=t.int64, device=eng.device)
    L.check(lib.tpe_rows_scatter(d_src.data_ptr(), d_rows.data_ptr(), count.data_ptr(), begin, win,
                                 dst.data_ptr(), ld, J.stream_ptr(eng)), "tpe_rows_scatter")
    assert (_bits(dst.cpu().numpy()) == _bits(want)).all()


def test_score_tree_device_keeps_the_groups_log_l_above():
    from tests.test_gpu_joint_tree import _nested
    domain, trials, pool, kw, ref = _nested()
    S = tpe.score_configs(domain, trials, pool, joint="tree", **kw)
    st = pool_mod._settings(kw["prior_weight"], kw["gamma"], 25, "tree", batch="liar-tree")
    _eng, d = pool_mod._score_device(domain, trials, pool, st, False)
    assert (_bits(d.S[:len(pool)].cpu().numpy()) == _bits(S)).all() and d.parts is None
    A, LA = d.above.cpu().numpy().T, ref[3]
    live = ~np.isnan(LA)
    assert live[:, 1:].any() and (np.abs(A[live] - LA[live]) <= 1e-6 * np.abs(LA[live])).all()


def test_public_path_on_a_quantized_branch_space():
    """Good trials at one point of branch 0; the pool is that branch's whole
    32 x 32 lattice and the 32 rows of branch 1."""
    space = {"v": hp.choice("v", [{"x": hp.quniform("x", 0, 31, 1), "y": hp.quniform("y", 0, 31, 1)},
                                  {"c": hp.quniform("c", 0, 31, 1)}])}
    domain, rng, at = Domain(lambda x: 0, space), np.random.RandomState(2), range(32)
    cfgs = [{"v": 0, "x": 12.0, "y": 20.0}] * 10
    cfgs += [{"v": 0, "x": float(a), "y": float(b)} for a, b in rng.randint(0, 32, (20, 2))]
    cfgs += [{"v": 1, "c": float(c)} for c in rng.randint(0, 32, 10)]
    trials = U.make_trials(domain, cfgs, [0.01 * i + (i >= 10) for i in range(40)])
    pool = tpe.Pool(domain, [{"v": 0, "x": float(x), "y": float(y)} for x in at for y in at] +
                    [{"v": 1, "c": float(c)} for c in at])
    hist = tpe.collect_history(trials, pool.labels)
    kw = dict(gamma=1.5)  # ceil(1.5 sqrt(40)) = 10 below rows: the good trials
    ref_rows, _at, _S = J.liar_tree_numpy(domain, hist, pool.vals, 8, pool.active, **kw)
    S0 = J.score_numpy(domain, hist, pool.vals, pool.active, tree=True, **kw)
    top = np.argsort(-S0, kind="stable")[:8]

    def spread(rows):
        v = np.nan_to_num(pool.vals[rows])
        return np.sqrt(((v[:, None, :] - v[None, :, :]) ** 2).sum(-1)).sum() / 56

    assert ref_rows[0] == top[0] < 1024 and spread(ref_rows) > spread(top)
    ids = list(range(500, 508))
    tpe.suggest_from_pool(ids, domain, trials, 0, pool=pool, joint="tree", batch="liar-tree",
                          verbose=False, **kw)
    assert [pool.row_of[i] for i in ids] == ref_rows.tolist()
    pool.release(ref_rows)
    # rows equal at the root: next to the pick and far from it; a row of the other branch
    p = int(ref_rows[0])
    near, far, other = p + 1, (p + 16 * 32 + 16) % 1024, 1030
    rows, _at, S_1 = tpe.pick_batch(domain, trials, pool, 1, return_trace=True, joint="tree", **kw)
    _rows, _at, root_1 = tpe.pick_batch(domain, trials, pool, 1, return_trace=True, **kw)
    pen = S0 - S_1
    root = tpe.score_configs(domain, trials, pool, joint=True, **kw) - root_1
    assert rows.tolist() == [p] and pen[near] > pen[far] > 0.0
    assert root[near] > 0.0 and abs(root[near] - root[far]) <= 1e-9 * root[near]
    assert 0.0 < pen[other] and abs(pen[other] - root[other]) <= 1e-9  # the root's lie alone
    tpe.suggest_from_pool(ids[:3], domain, trials, 7, pool=pool, joint="tree", batch="liar-tree",
                          n_startup_jobs=10 ** 6, verbose=False)
    got = [pool.row_of[i] for i in ids[:3]]
    pool.release(got)
    assert got == pool_mod.startup_rows(pool, 7, 3).tolist()
    # a sampled pool: k distinct documents, none of them a trial; fmin with a queue
    skw = dict(n_EI_candidates=512, joint="tree", draw="joint", batch="liar-tree", verbose=False)
    docs = tpe.suggest_sampled(ids[:6], domain, trials, 21, distinct=True, **skw)
    got = {tuple(sorted((lab, float(v[0])) for lab, v in d["misc"]["vals"].items() if v))
           for d in docs}
    assert len(docs) == 6 == len(got)
    assert not got & {tuple(sorted((lab, float(v)) for lab, v in c.items())) for c in cfgs}
    trials = Trials()
    fmin(lambda cfg: abs(cfg["v"].get("x", 30.0) - 12.0), space, max_evals=40, max_queue_len=4,
         algo=functools.partial(tpe.suggest_sampled, **skw), trials=trials,
         rstate=np.random.RandomState(0), show_progressbar=False)
    assert len(trials) == 40
