"""``joint="tree"`` on the host: the groups, the numpy form against the scalar
restatement of tests/joint_tree_util.py, the keys, and the argument errors
that need no device.

Values: |got - ref| <= 1e-6 * sum over the live groups of (|log L_below,g| +
|log L_above,g|), as tests/test_gpu_joint.py applies the project's fp64
log-density tolerance; NaN positions and every "same bits" statement exactly.
"""
import numpy as np
import pytest

from hyperopt_amd import Domain, hp, rand, tpe
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from tests import joint_tree_util as TU
from tests import joint_util as U


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.shape(a) == np.shape(b) and (_bits(a) == _bits(b)).all()


def _groups(domain):
    return [(g.clauses, g.labels) for g in J.joint_groups(domain)]


# -- 1. groups -------------------------------------------------------------------
def test_groups_of_the_nested_case():
    domain = TU.nested_case()[0]
    assert [labs for _c, labs in _groups(domain)] == [
        ["root"], ["lin_lr"], ["tree_depth", "tree_split"], ["gini_w"], ["ent_s", "ent_w"],
        ["nn_drop", "nn_units"]]
    assert _groups(domain) == TU.groups_of(domain)
    assert _groups(domain)[0] == (((),), J.joint_labels(domain))
    assert _groups(domain)[3][0] == ((("root", 1), ("tree_split", 0)),)
    assert tpe.joint_groups is J.joint_groups


def test_groups_two_clauses_and_two_levels():
    domain = Domain(lambda x: 0, TU.two_clause_space())
    got = {tuple(labs): clauses for clauses, labs in _groups(domain)}
    assert _groups(domain) == TU.groups_of(domain)
    params = list(domain.params)
    for labs in got:  # labels in params order, groups by their first label
        assert list(labs) == sorted(labs, key=params.index)
    firsts = [params.index(labs[0]) for _c, labs in _groups(domain)]
    assert firsts == sorted(firsts)
    assert sorted(sum((list(labs) for labs in got), [])) == sorted(params)
    assert got[("free", "s")] == ((),) or got[("s", "free")] == ((),)
    assert got[("w",)] == ((("s", 0),), (("s", 1),))          # reachable from two branches
    assert got[("x", "y")] == ((("s", 0),),)                  # identical clauses: one group
    assert got[("t",)] == ((("s", 1),),)
    assert got[("z",)] == ((("s", 1), ("t", 0)),)             # two levels down
    assert got[("zz",)] == ((("s", 1), ("t", 1)),)
    assert got[("lone",)] == ((("s", 2),),)


def test_flat_space_has_one_group():
    domain = Domain(lambda x: 0, U.all_kinds_space(hp))
    assert _groups(domain) == [(((),), J.joint_labels(domain))]
    assert J.joint_labels(domain) == list(domain.params)


def test_switch_on_an_expression_raises():
    from hyperopt_amd.pyll import scope
    a, b = hp.randint("a", 2), hp.randint("b", 2)
    space = scope.switch(a + b, hp.uniform("x", 0, 1), hp.uniform("y", 0, 1), hp.uniform("z", 0, 1))
    domain = Domain(lambda x: 0, space)
    assert domain.live_program() is None
    with pytest.raises(ValueError, match="switch"):
        J.joint_groups(domain)
    assert J.joint_labels(domain) == ["a", "b"]   # (joint=True still has its labels)
    empty = Domain(lambda x: 0, {"x": 1.0})
    with pytest.raises(ValueError, match="joint"):
        J.joint_groups(empty)


# -- 2. the numpy form -----------------------------------------------------------
def _numpy_tree(domain, trials, pool, **kw):
    hist = tpe.collect_history(trials, pool.labels)
    return J.score_numpy(domain, hist, pool.vals, pool.active, tree=True, return_parts=True, **kw)


def _check_against_restatement(domain, trials, pool, kw):
    S, Jm, LB, LA = _numpy_tree(domain, trials, pool, **kw)
    ref = TU.tree_reference(domain, trials, pool.vals, pool.active,
                            prior_weight=kw.get("prior_weight", 1.0), gamma=kw.get("gamma", 0.25))
    rS, rJ, rLB, rLA, ns = ref
    live = TU.group_live(domain, pool.active)
    np.testing.assert_array_equal(np.isnan(Jm), np.isnan(rJ))
    np.testing.assert_array_equal(np.isnan(LB), ~live)
    tol = TU.tolerance(rLB, rLA)
    fin = ~np.isnan(rS)
    np.testing.assert_array_equal(np.isnan(S), ~fin)
    assert (np.abs(S[fin] - rS[fin]) <= tol[fin]).all()
    for g in range(Jm.shape[1]):
        on = live[:, g] & ~np.isnan(rJ[:, g])
        assert (np.abs(Jm[on, g] - rJ[on, g]) <= 1e-6 * (np.abs(rLB[on, g]) +
                                                         np.abs(rLA[on, g]))).all()
    assert _same_bits(S, TU.fold_live(Jm, live))     # S is the fold of the parts
    return S, ns


def test_score_numpy_tree_matches_the_restatement_on_the_nested_case():
    domain, trials, pool, kw = TU.nested_case()
    S, ns = _check_against_restatement(domain, trials, pool, kw)
    assert np.isfinite(S).all() and len(ns) == 6
    assert all(nb + na > 0 for nb, na in ns)
    hist = tpe.collect_history(trials, pool.labels)
    plain = J.score_numpy(domain, hist, pool.vals, pool.active, **kw)
    assert not _same_bits(S, plain)                  # the other groups add to J_root
    # without return_parts: the same S
    assert _same_bits(J.score_numpy(domain, hist, pool.vals, pool.active, tree=True, **kw), S)
    # active=None reads the liveness off the NaNs of Pool.vals
    assert _same_bits(J.score_numpy(domain, hist, pool.vals, tree=True, **kw), S)


@pytest.mark.parametrize("name", sorted(TU.edge_histories()))
def test_score_numpy_tree_edges(name):
    domain = Domain(lambda x: 0, TU.branch_space())
    configs, losses = TU.edge_histories()[name]
    trials = U.make_trials(domain, configs, losses)
    pool = tpe.Pool(domain, TU.branch_pool_rows())
    S, ns = _check_against_restatement(domain, trials, pool, {})
    ab = ns[1]  # the group (a, b); the foreign trial is the best one, and it is left out
    assert ab == {"never_tried": (0, 0), "above_only": (0, 4), "foreign_half": (0, 4),
                  "empty": (0, 0)}[name]
    if name == "empty":
        assert (S == 0.0).all()


def test_flat_tree_has_the_bits_of_the_default():
    domain = Domain(lambda x: 0, U.all_kinds_space(hp))
    rng = np.random.RandomState(3)
    configs = [rand.sample_config(domain, rng) for _ in range(40)]
    trials = U.make_trials(domain, configs, rng.uniform(size=40))
    pool = tpe.Pool(domain, [rand.sample_config(domain, rng) for _ in range(33)])
    hist = tpe.collect_history(trials, pool.labels)
    plain = J.score_numpy(domain, hist, pool.vals, pool.active)
    S, Jm, LB, LA = J.score_numpy(domain, hist, pool.vals, pool.active, tree=True,
                                  return_parts=True)
    assert _same_bits(S, plain) and Jm.shape == (33, 1) and _same_bits(Jm[:, 0], plain)


def test_the_diagonal_of_branch_0_scores_above_the_rest_in_numpy():
    """The ranking case of tests/test_gpu_joint_tree.py is chosen here, on the
    CPU: every diagonal row of branch 0 scores above every off-diagonal one."""
    domain, trials = TU.branch_diagonal_case()
    hist = tpe.collect_history(trials, list(domain.params))
    isb, _ = tpe.split_masks(hist, TU.GAMMA_DIAGONAL)
    assert isb.sum() == 16
    pool = tpe.Pool(domain, TU.branch_pool_rows())
    S = J.score_numpy(domain, hist, pool.vals, pool.active, gamma=TU.GAMMA_DIAGONAL, tree=True)
    diag = np.asarray([0, 5, 10, 15])
    off = np.setdiff1d(np.arange(16), diag)
    assert S[diag].min() > S[off].max()
    assert S[diag].min() > S[16]
    plain = J.score_numpy(domain, hist, pool.vals, pool.active, gamma=TU.GAMMA_DIAGONAL)
    assert (plain[:16] == plain[0]).all()            # joint=True sees the selector alone


# -- 3. keys ---------------------------------------------------------------------
def test_group_component_keys_are_distinct():
    for domain in (TU.nested_case()[0], Domain(lambda x: 0, TU.two_clause_space())):
        for seed in (0, 1, 123, 2 ** 31 - 1):
            groups = J.joint_groups(domain)
            keys = [J.group_component_key(seed, g.labels[0]) for g in groups[1:]]
            labels = [tpe.label_key(seed, lab) for lab in domain.params]
            every = keys + [J.component_key(seed)] + labels
            assert len(set(every)) == len(every)
            assert all(0 <= k < 2 ** 64 for k in keys)
            assert keys[0] == tpe._mix64(tpe.label_key(seed, groups[1].labels[0]) ^ J.STREAM_JOINT)
    assert tpe.joint_group_component_key is J.group_component_key


# -- 4. argument errors that need no device ----------------------------------------
def test_argument_errors():
    domain, trials = TU.branch_diagonal_case()
    pool = tpe.Pool(domain, TU.branch_pool_rows())
    with pytest.raises(ValueError, match="bandwidth"):
        tpe.score_configs(domain, trials, pool, joint="tree", bandwidth=0.0)
    with pytest.raises(ValueError, match="cat_smoothing"):
        tpe.suggest_from_pool([1], domain, trials, 0, pool=pool, joint="tree", cat_smoothing=-1.0,
                              verbose=False)
    with pytest.raises(ValueError, match="joint"):
        tpe.suggest_sampled([1], domain, trials, 0, draw="joint", verbose=False)
    with pytest.raises(ValueError, match="draw"):
        tpe.suggest_sampled([1], domain, trials, 0, joint="tree", draw="tree", verbose=False)
    grid = tpe.GridPool(domain, {"v": [0, 1], "a": [0, 1, 2, 3], "b": [0, 1, 2, 3], "c": [0.5]})
    with pytest.raises(ValueError, match="to_pool"):
        tpe.score_configs(domain, trials, grid, joint="tree")
    with pytest.raises(ValueError, match="to_pool"):
        tpe.suggest_from_pool([1], domain, trials, 0, pool=grid, joint="tree", verbose=False)
    # only the string "tree" changes meaning
    assert pool_mod._joint_kw("tree", 0.2, 1.0)["tree"] is True
    for other in (True, 1, "yes", "Tree", np.True_):
        assert pool_mod._joint_kw(other, 0.2, 1.0)["tree"] is False
    for off in (False, 0, None, ""):
        assert pool_mod._joint_kw(off, 0.2, 1.0) is None
    hist = tpe.collect_history(trials, pool.labels)
    bad = pool.active.copy()
    bad[0, list(domain.params).index("b")] = False   # half of group (a, b) in row 0
    with pytest.raises(ValueError, match="together"):
        J.score_numpy(domain, hist, pool.vals, bad, tree=True)
