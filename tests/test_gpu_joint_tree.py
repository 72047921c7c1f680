"""``joint="tree"`` on the GPU, through the public functions: one joint Parzen
mixture per group of labels that share an activation condition
(hyperopt_amd/joint.py "Groups", csrc/tpe_joint_tree.hip).

Values are checked against the scalar restatement of tests/joint_tree_util.py:
|got - ref| <= 1e-6 * sum over the live groups of (|log L_below,g| +
|log L_above,g|), the project's fp64 log-density tolerance as
tests/test_gpu_joint.py applies it.  -inf / NaN positions, orders and every
"same bits" statement are exact.  Drawn columns follow the numpy replay of
tests/joint_sample_util.py under tests/stream_cases.py's fp64 rules.
"""
import numpy as np
import pytest

from hyperopt_amd import Domain, tpe
from hyperopt_amd import _lib as L
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from tests import cond_util as C
from tests import joint_sample_util as R
from tests import joint_tree_util as TU
from tests import joint_util as U
from tests.test_gpu_pool import _expected_order

pytestmark = pytest.mark.gpu

SEED = 123
_SHARED = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.shape(a) == np.shape(b) and (_bits(a) == _bits(b)).all()


def _nested():
    """The nested case and its reference, computed once."""
    if "nested" not in _SHARED:
        domain, trials, pool, kw = TU.nested_case()
        ref = TU.tree_reference(domain, trials, pool.vals, pool.active, **kw)
        _SHARED["nested"] = (domain, trials, pool, kw, ref)
    return _SHARED["nested"]


def _check_values(domain, trials, pool, kw, ref):
    S, terms, Jm = tpe.score_configs(domain, trials, pool, joint="tree", return_terms=True, **kw)
    rS, rJ, rLB, rLA, _ns = ref
    live = TU.group_live(domain, pool.active)
    assert Jm.shape == rJ.shape and np.isnan(terms).all() and terms.shape == pool.vals.shape
    np.testing.assert_array_equal(np.isnan(Jm), np.isnan(rJ))
    assert not np.isnan(rJ[live]).any()
    np.testing.assert_array_equal(np.isnan(Jm), ~live)       # NaN exactly where not live
    assert _same_bits(S, TU.fold_live(Jm, live))             # S is the fold of J's columns
    err = np.abs(S - rS)
    tol = TU.tolerance(rLB, rLA)
    print("max |S - S_ref| = %.3g (tolerance there %.3g)" % (err.max(), tol[err.argmax()]))
    assert (err <= tol).all()
    for g in range(Jm.shape[1]):
        on = live[:, g]
        assert (np.abs(Jm[on, g] - rJ[on, g]) <= 1e-6 * (np.abs(rLB[on, g]) +
                                                         np.abs(rLA[on, g]))).all()
    assert _same_bits(tpe.score_configs(domain, trials, pool, joint="tree", **kw), S)
    return S, Jm


# -- 1. values -------------------------------------------------------------------
def test_values_on_the_nested_case():
    domain, trials, pool, kw, ref = _nested()
    live = TU.group_live(domain, pool.active)
    assert live.shape[1] == 6 and live[:, 1:].any(0).all() and not live[:, 1:].all(0).any()
    S, Jm = _check_values(domain, trials, pool, kw, ref)
    # "tree" is not read as True: the groups under the switch are in S
    plain = tpe.score_configs(domain, trials, pool, joint=True, **kw)
    assert not _same_bits(S, plain)
    # the root group's column is joint=True's J
    _, _, Jroot = tpe.score_configs(domain, trials, pool, joint=True, return_terms=True, **kw)
    assert _same_bits(Jm[:, 0], Jroot)
    # and the numpy form agrees
    hist = tpe.collect_history(trials, pool.labels)
    Sn = J.score_numpy(domain, hist, pool.vals, pool.active, tree=True, **kw)
    assert (np.abs(S - Sn) <= TU.tolerance(ref[2], ref[3])).all()


def test_flat_space_has_the_bits_of_joint_true():
    from tests.test_gpu_joint import KW, _all_kinds
    domain, trials, pool, _ = _all_kinds()
    plain = tpe.score_configs(domain, trials, pool, joint=True, **KW)
    S, terms, Jm = tpe.score_configs(domain, trials, pool, joint="tree", return_terms=True, **KW)
    assert _same_bits(S, plain) and np.isnan(terms).all()
    assert Jm.shape == (len(pool), 1) and _same_bits(Jm[:, 0], plain)
    np.testing.assert_array_equal(np.flatnonzero(np.isnan(S)), [5, 299])


# -- 2. invariance ---------------------------------------------------------------
def test_bits_do_not_depend_on_pool_shape_window_or_call(monkeypatch):
    domain, trials, pool, kw, _ = _nested()
    whole = tpe.score_configs(domain, trials, pool, joint="tree", **kw)
    assert _same_bits(tpe.score_configs(domain, trials, pool, joint="tree", **kw), whole)
    sub = np.random.RandomState(2).permutation(len(pool))[:137]
    small = tpe.Pool.from_arrays(domain, pool.vals[sub], pool.active[sub])
    assert _same_bits(tpe.score_configs(domain, trials, small, joint="tree", **kw), whole[sub])
    monkeypatch.setattr(J, "ROWS_PER_CALL", 128)  # list windows [0, 128) [128, 256) [256, 300)
    fresh = tpe.Pool.from_arrays(domain, pool.vals, pool.active)
    S, _, Jm = tpe.score_configs(domain, trials, fresh, joint="tree", return_terms=True, **kw)
    assert _same_bits(S, whole)
    assert _same_bits(S, TU.fold_live(Jm, TU.group_live(domain, pool.active)))


# -- 3. edges --------------------------------------------------------------------
def test_a_group_live_in_no_pool_row():
    domain, trials = TU.branch_diagonal_case()
    pool = tpe.Pool(domain, [{"v": 1, "c": 0.05 * (i + 1)} for i in range(19)])
    kw = dict(gamma=TU.GAMMA_DIAGONAL)
    ref = TU.tree_reference(domain, trials, pool.vals, pool.active, **kw)
    _, Jm = _check_values(domain, trials, pool, kw, ref)
    assert np.isnan(Jm[:, 1]).all() and not np.isnan(Jm[:, [0, 2]]).any()


@pytest.mark.parametrize("name", sorted(TU.edge_histories()))
def test_edge_histories(name):
    """A branch never tried (prior alone on both sides), tried only above, a
    foreign trial with half a group's labels, no trials at all."""
    domain = Domain(lambda x: 0, TU.branch_space())
    configs, losses = TU.edge_histories()[name]
    trials = U.make_trials(domain, configs, losses)
    pool = tpe.Pool(domain, TU.branch_pool_rows())
    ref = TU.tree_reference(domain, trials, pool.vals, pool.active)
    assert ref[4][1] == {"never_tried": (0, 0), "above_only": (0, 4), "foreign_half": (0, 4),
                         "empty": (0, 0)}[name]
    S, Jm = _check_values(domain, trials, pool, {}, ref)
    if name in ("never_tried", "empty"):  # both sets are the prior: J_g is exactly 0
        assert (Jm[:16, 1] == 0.0).all()
    if name == "empty":
        assert (S == 0.0).all()


# -- 4. ranking ------------------------------------------------------------------
def test_suggest_from_pool_ranks_the_diagonal_of_the_branch_first():
    domain, trials = TU.branch_diagonal_case()
    rows = TU.branch_pool_rows()
    kw = dict(gamma=TU.GAMMA_DIAGONAL, verbose=False)
    # (that the numpy form ranks the diagonal first: tests/test_joint_tree_host.py)
    hist = tpe.collect_history(trials, list(domain.params))
    pool = tpe.Pool(domain, rows)
    Sn = J.score_numpy(domain, hist, pool.vals, pool.active, gamma=TU.GAMMA_DIAGONAL, tree=True)
    assert Sn[[0, 5, 10, 15]].min() > np.delete(Sn, [0, 5, 10, 15]).max()
    ids = [100, 101, 102, 103]
    docs = tpe.suggest_from_pool(ids, domain, trials, 0, pool=pool, joint="tree", **kw)
    assert len(docs) == 4 and {pool.row_of[i] for i in ids} == {0, 5, 10, 15}
    for doc in docs:
        assert doc["misc"]["vals"]["a"] == doc["misc"]["vals"]["b"]
        assert doc["misc"]["vals"]["v"] == [0] and doc["misc"]["vals"]["c"] == []
    S = tpe.score_configs(domain, trials, pool, gamma=TU.GAMMA_DIAGONAL, joint="tree")
    assert [pool.row_of[i] for i in ids] == _expected_order(S, np.zeros(17), 4).tolist()
    # joint=True sees the selector alone and does not find the diagonal
    flat = tpe.Pool(domain, rows)
    tpe.suggest_from_pool(ids, domain, trials, 0, pool=flat, joint=True, **kw)
    assert {flat.row_of[i] for i in ids} != {0, 5, 10, 15}
    # distinct: every configuration of branch 0 is in the history
    twice = tpe.Pool(domain, rows + rows)
    fresh = tpe.suggest_from_pool(ids, domain, trials, 0, pool=twice, joint="tree", distinct=True,
                                  **kw)
    assert [twice.row_of[d["tid"]] for d in fresh] == [16]   # (c = 0.5 is new; once)


# -- 5. sampling -----------------------------------------------------------------
def _group_replay(domain, hist, seed, grp, n, g_index, **kw):
    """The numpy replay of one group's columns: tests/joint_sample_util.py on
    the group's below set, labels and keys."""
    models = J.label_models(domain, grp.labels)
    cols = [m.col for m in models]
    isb = tpe.split_masks(hist, kw.get("gamma", 0.25))[0]
    rows = J.set_rows(hist, isb, cols)
    mu = np.zeros((len(models), rows.size))
    for d, m in enumerate(models):
        obs = np.asarray(hist.vals)[rows, m.col]
        if m.kind == L.JOINT_CAT:
            mu[d] = np.rint(obs) - m.offset
        else:
            mu[d] = np.log(np.maximum(obs, R.EPS)) if m.is_log else obs
    cdf = np.cumsum(np.concatenate([J.forgetting_weights(rows.size, 25),
                                    [float(kw.get("prior_weight", 1.0))]]))
    sig = J.bandwidths(models, rows.size, J.BANDWIDTH)
    keys = [tpe.label_key(seed, m.label) for m in models]
    if g_index == 0:
        comp_key = J.component_key(seed)
    else:  # (written out: the rule of the module text, not the package's function)
        comp_key = tpe._mix64(tpe.label_key(seed, grp.labels[0]) ^ 0x4A4F494E)
    _comp, out = R.replay_set(models, mu, sig, cdf, keys, comp_key, 1.0 + J.CAT_SMOOTHING,
                              np.arange(n))
    return models, out


@pytest.mark.parametrize("n", [300, 4096])
def test_pool_sample_tree(n):
    domain, trials, _pool, kw, _ = _nested()
    labels = list(domain.params)
    hist = tpe.collect_history(trials, labels)
    pool = tpe.Pool.sample(domain, trials, SEED, n, joint="tree", keep_terms=True, **kw)
    assert isinstance(pool, tpe.SampledPool) and len(pool) == n
    dv = pool._born().vals[:, :n].cpu().numpy()
    groups = J.joint_groups(domain)
    # the root group's columns: the bits of joint=True
    plain = tpe.Pool.sample(domain, trials, SEED, n, joint=True, **kw)
    root = [labels.index(lab) for lab in groups[0].labels]
    assert _same_bits(dv[root], plain._born().vals[:, :n].cpu().numpy()[root])
    # every group's columns (all the rows are drawn): the numpy replay
    left_out = 0
    for g, grp in enumerate(groups):
        models, out = _group_replay(domain, hist, SEED, grp, n, g, **kw)
        for m, rep in zip(models, out):
            left_out += R.compare(m, rep, dv[m.col])[1]
    print("n = %d: %d ambiguous entries left out" % (n, left_out))
    # activity: the space's program on the drawn selectors; the pool validates
    active, vals = pool.active, pool.vals
    lo, co, tm = pool_mod.program_csr(domain)
    np.testing.assert_array_equal(active.T, C.interpret(lo, co, tm, dv, n))
    tpe.Pool.from_arrays(domain, vals, active)
    assert np.isnan(pool.terms()).all()                      # every label is joint
    # born with the tree S of its own rows
    born = pool.scores().copy()
    assert np.isfinite(born).all()
    S, _, Jm = tpe.score_configs(domain, trials, pool, joint="tree", return_terms=True, **kw)
    assert _same_bits(born, S)
    assert _same_bits(S, TU.fold_live(Jm, TU.group_live(domain, active)))
    if n == 300:
        ref = TU.tree_reference(domain, trials, vals, active, **kw)
        assert (np.abs(born - ref[0]) <= TU.tolerance(ref[2], ref[3])).all()
        twin = tpe.Pool.sample(domain, trials, SEED, n, joint="tree", **kw)
        assert _same_bits(twin._born().vals[:, :n].cpu().numpy(), dv)
        assert _same_bits(twin.scores(), born)


def test_share_of_the_diagonal_within_the_branch():
    """The group (a, b)'s below set is the 16 diagonal trials plus the prior:
    a trial component puts 0.625^2 + 3 x 0.125^2 = 0.4375 on a == b, the prior
    0.25, so (16 x 0.4375 + 0.25) / 17 = 0.4265 of the rows with v == 0 lie on
    the diagonal (DESIGN 3.5.5's derivation); within 4 binomial standard
    deviations at the number of such rows."""
    domain, trials = TU.branch_diagonal_case()
    labels = list(domain.params)
    n = 4096
    pool = tpe.Pool.sample(domain, trials, SEED, n, joint="tree", gamma=TU.GAMMA_DIAGONAL)
    dv = pool._born().vals[:, :n].cpu().numpy()
    v, a, b = (dv[labels.index(lab)] for lab in ("v", "a", "b"))
    on = v == 0
    m = int(on.sum())
    assert m > 1000
    np.testing.assert_array_equal(pool.active[:, labels.index("a")], on)
    share = float((a[on] == b[on]).mean())
    p = 0.4265
    sd = np.sqrt(p * (1.0 - p) / m)
    print("on the diagonal: %.4f of %d rows (sd %.4f)" % (share, m, sd))
    assert abs(share - p) <= 4.0 * sd
    assert _same_bits(pool.scores(), tpe.score_configs(domain, trials, pool, joint="tree",
                                                       gamma=TU.GAMMA_DIAGONAL))


def _doc_config(doc):
    return {k: v[0] for k, v in doc["misc"]["vals"].items() if v}


def test_suggest_sampled_tree():
    domain, trials = TU.branch_diagonal_case()
    ids = [200, 201, 202, 203, 204]
    kw = dict(n_EI_candidates=256, gamma=TU.GAMMA_DIAGONAL, verbose=False)
    # draw="joint": the k best rows of Pool.sample(joint="tree") by its born S
    docs = tpe.suggest_sampled(ids, domain, trials, SEED, joint="tree", draw="joint", **kw)
    pool = tpe.Pool.sample(domain, trials, SEED, 256, joint="tree", gamma=TU.GAMMA_DIAGONAL)
    rows = _expected_order(pool.scores(), np.zeros(256), len(ids))
    assert [d["tid"] for d in docs] == ids
    assert [_doc_config(d) for d in docs] == [pool.config(int(r)) for r in rows]
    # distinct: k valid documents, pairwise distinct, none of them in the history
    fresh = tpe.suggest_sampled(ids, domain, trials, SEED, joint="tree", draw="joint",
                                distinct=True, **kw)
    cfgs = [_doc_config(d) for d in fresh]
    assert len(cfgs) == len(ids)
    assert len({tuple(sorted(c.items())) for c in cfgs}) == len(cfgs)
    for c in cfgs:  # (branch 0 is used up: fresh rows are of branch 1, with a new c)
        assert set(c) == {"v", "c"} and c["v"] == 1 and 0.0 <= c["c"] <= 1.0
    tpe.Pool(domain, cfgs)                                   # valid configurations
    # the default draw samples as today and ranks by the tree S
    docs = tpe.suggest_sampled(ids, domain, trials, SEED, joint="tree", **kw)
    plain = tpe.Pool.sample(domain, trials, SEED, 256, gamma=TU.GAMMA_DIAGONAL)
    S = tpe.score_configs(domain, trials, plain, joint="tree", gamma=TU.GAMMA_DIAGONAL)
    rows = _expected_order(S, np.zeros(256), len(ids))
    assert [_doc_config(d) for d in docs] == [plain.config(int(r)) for r in rows]
    # draw="joint" without a joint option still raises
    with pytest.raises(ValueError, match="joint"):
        tpe.suggest_sampled(ids, domain, trials, SEED, draw="joint", **kw)
    # the startup phase is today's
    start = dict(n_EI_candidates=64, n_startup_jobs=101, verbose=False)
    d1 = tpe.suggest_sampled(ids, domain, trials, 9, joint="tree", draw="joint", **start)
    d2 = tpe.suggest_sampled(ids, domain, trials, 9, **start)
    assert [d["misc"]["vals"] for d in d1] == [d["misc"]["vals"] for d in d2]
    a, b = tpe.Pool(domain, TU.branch_pool_rows()), tpe.Pool(domain, TU.branch_pool_rows())
    tpe.suggest_from_pool(ids[:3], domain, trials, 9, pool=a, joint="tree", n_startup_jobs=101,
                          verbose=False)
    tpe.suggest_from_pool(ids[:3], domain, trials, 9, pool=b, n_startup_jobs=101, verbose=False)
    assert [a.row_of[i] for i in ids[:3]] == [b.row_of[i] for i in ids[:3]]
