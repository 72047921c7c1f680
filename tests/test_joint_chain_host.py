"""``joint="chain"`` on the host: the contexts, the numpy form against the
scalar restatement of tests/joint_chain_util.py, the settings and the argument
checks of tpe_joint_chain_rows that need no device.

Values: |got - ref| <= 1e-6 * sum over the live groups of (|log L_below| +
|log L_above|, plus the two context marginals' |.| for a group with a context),
the project's fp64 log-density rule as tests/joint_tree_util.py applies it; NaN
positions and every "same bits" statement exactly.
"""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import Domain, hp, rand, tpe
from hyperopt_amd import _lib as L
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from tests import joint_chain_util as CU
from tests import joint_tree_util as TU
from tests import joint_util as U


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.shape(a) == np.shape(b) and (_bits(a) == _bits(b)).all()


def _by_first(domain):
    """{first label of the group: its context}"""
    return {g.labels[0]: ctx for g, ctx in zip(J.joint_groups(domain), J.joint_contexts(domain))}


# -- 1. contexts -----------------------------------------------------------------
def test_contexts_of_the_two_clause_space():
    domain = Domain(lambda x: 0, TU.two_clause_space())
    params = list(domain.params)
    got = _by_first(domain)
    root = J.joint_labels(domain)
    assert sorted(root) == ["free", "s"] and got[root[0]] == []

    def ordered(labs):
        return sorted(labs, key=params.index)
    assert got["w"] == ordered(["s", "free"])             # two branches: the selector varies
    assert got["x"] == ordered(["free", "w"])             # under (s, 0): s is fixed, w is live
    assert got["t"] == ordered(["free", "w"])
    assert got["z"] == ordered(["free", "w"])             # s and t fixed; t's group holds t alone
    assert got["zz"] == ordered(["free", "w"])
    assert got["lone"] == ["free"]                        # w is not live under (s, 2)
    assert J.joint_contexts(domain) == CU.contexts_of(domain)
    assert tpe.joint_contexts is J.joint_contexts


def test_contexts_of_the_nested_case():
    domain = TU.nested_case()[0]
    got = _by_first(domain)
    # the root group is the selector alone, fixed under every branch; a nested
    # group holds its ancestor group's labels without the fixed selectors
    assert got == {"root": [], "lin_lr": [], "tree_depth": [], "gini_w": ["tree_depth"],
                   "ent_s": ["tree_depth"], "nn_drop": []}
    assert J.joint_contexts(domain) == CU.contexts_of(domain)


def test_contexts_empty_on_branch_space_and_flat():
    domain = Domain(lambda x: 0, TU.branch_space())
    assert J.joint_contexts(domain) == [[], [], []] == CU.contexts_of(domain)
    flat = Domain(lambda x: 0, U.all_kinds_space(hp))
    assert J.joint_contexts(flat) == [[]]
    cross = Domain(lambda x: 0, CU.cross_space())
    assert _by_first(cross) == {J.joint_labels(cross)[0]: [], "b": ["a"], "c": ["a"]}


# -- 2. the numpy form -----------------------------------------------------------
def _check_against_restatement(domain, trials, pool, kw):
    hist = tpe.collect_history(trials, pool.labels)
    got = J.score_numpy(domain, hist, pool.vals, pool.active, tree="chain", return_parts=True, **kw)
    assert len(got) == 6
    S, Cm = got[0], got[1]
    ref = CU.chain_reference(domain, trials, pool.vals, pool.active,
                             prior_weight=kw.get("prior_weight", 1.0), gamma=kw.get("gamma", 0.25))
    live = TU.group_live(domain, pool.active)
    contexts = J.joint_contexts(domain)
    for m, r in zip(got[1:], ref[1:6]):
        np.testing.assert_array_equal(np.isnan(m), np.isnan(r))
    np.testing.assert_array_equal(np.isnan(got[2]), ~live)
    for g, ctx in enumerate(contexts):  # the marginals: live rows of the groups with a context
        np.testing.assert_array_equal(np.isnan(got[4][:, g]), ~live[:, g] | (not ctx))
    tol = CU.tolerance(*ref[2:6])
    err = np.abs(S - ref[0])
    print("max |S - S_ref| = %.3g (tolerance there %.3g)" % (err.max(), tol[err.argmax()]))
    assert (err <= tol).all()
    for g in range(Cm.shape[1]):
        on = live[:, g]
        assert (np.abs(Cm[on, g] - ref[1][on, g]) <= CU.column_tolerance(ref, g)[on]).all()
        for m, r in zip(got[2:], ref[2:6]):
            fin = on & ~np.isnan(r[:, g])
            assert (np.abs(m[fin, g] - r[fin, g]) <= 1e-6 * np.abs(r[fin, g])).all()
    assert _same_bits(S, TU.fold_live(Cm, live))              # S is the fold of C
    assert _same_bits(J.score_numpy(domain, hist, pool.vals, pool.active, tree="chain", **kw), S)
    return S, ref


def test_score_numpy_chain_on_the_cross_level_case():
    domain, trials = CU.cross_level_case()
    pool = tpe.Pool(domain, CU.cross_pool_rows())
    S, ref = _check_against_restatement(domain, trials, pool, dict(gamma=TU.GAMMA_DIAGONAL))
    assert ref[6][1] == (16, 48)                              # (a, b): the diagonal below
    order = np.argsort(-S, kind="stable")
    assert sorted(order[:4]) == CU.DIAGONAL
    assert S[order[3]] - S[order[4]] > 0.5
    # the reference itself ranks the diagonal first, by a wide gap ...
    rS = ref[0]
    assert np.delete(rS, CU.DIAGONAL).max() < rS[CU.DIAGONAL].min() - 0.5
    # ... and the independent groups of "tree" do not: flat in b for a fixed a
    hist = tpe.collect_history(trials, pool.labels)
    tree = J.score_numpy(domain, hist, pool.vals, pool.active, tree=True, gamma=TU.GAMMA_DIAGONAL)
    assert sorted(np.argsort(-tree, kind="stable")[:4]) != CU.DIAGONAL
    assert np.ptp(tree[:16].reshape(4, 4), axis=1).max() < 0.2
    assert not _same_bits(S, tree)


def test_score_numpy_chain_on_the_two_clause_space():
    domain = Domain(lambda x: 0, TU.two_clause_space())
    rng = np.random.RandomState(7)
    configs = [rand.sample_config(domain, rng) for _ in range(120)]
    trials = U.make_trials(domain, configs, rng.uniform(size=120))
    pool = tpe.Pool(domain, [rand.sample_config(domain, rng) for _ in range(60)])
    S, ref = _check_against_restatement(domain, trials, pool, {})
    live = TU.group_live(domain, pool.active)
    assert live[:, 1:].any(0).all()                           # every group is live somewhere
    assert np.isfinite(S).all()


def test_empty_contexts_have_the_bits_of_tree_and_flat_of_the_default():
    domain, trials = TU.branch_diagonal_case()
    pool = tpe.Pool(domain, TU.branch_pool_rows())
    hist = tpe.collect_history(trials, pool.labels)
    kw = dict(gamma=TU.GAMMA_DIAGONAL)
    tree = J.score_numpy(domain, hist, pool.vals, pool.active, tree=True, return_parts=True, **kw)
    chain = J.score_numpy(domain, hist, pool.vals, pool.active, tree="chain", return_parts=True,
                          **kw)
    for a, b in zip(tree, chain[:4]):
        assert _same_bits(a, b)
    assert np.isnan(chain[4]).all() and np.isnan(chain[5]).all()
    flat = Domain(lambda x: 0, U.all_kinds_space(hp))
    rng = np.random.RandomState(3)
    trials = U.make_trials(flat, [rand.sample_config(flat, rng) for _ in range(40)],
                           rng.uniform(size=40))
    pool = tpe.Pool(flat, [rand.sample_config(flat, rng) for _ in range(33)])
    hist = tpe.collect_history(trials, pool.labels)
    assert _same_bits(J.score_numpy(flat, hist, pool.vals, pool.active, tree="chain"),
                      J.score_numpy(flat, hist, pool.vals, pool.active))


# -- 3. settings -----------------------------------------------------------------
def test_settings():
    kw = pool_mod._joint_kw("chain", 0.2, 1.0)
    assert kw == dict(bandwidth=0.2, cat_smoothing=1.0, tree="chain")    # a value, not a key
    assert pool_mod._joint_kw("tree", 0.2, 1.0)["tree"] is True
    for other in (True, 1, "yes", "Chain", "chains"):
        assert pool_mod._joint_kw(other, 0.2, 1.0)["tree"] is False
    domain, trials = CU.cross_level_case()
    pool = tpe.Pool(domain, CU.cross_pool_rows())
    with pytest.raises(ValueError, match="bandwidth"):
        tpe.score_configs(domain, trials, pool, joint="chain", bandwidth=0.0)
    # the liar batch
    for call in (lambda: pool_mod._settings(1.0, 0.25, 25, "chain", batch="liar"),
                 lambda: tpe.suggest_from_pool([1], domain, trials, 0, pool=pool, joint="chain",
                                               batch="liar", verbose=False),
                 lambda: tpe.suggest_sampled([1], domain, trials, 0, joint="chain", batch="liar",
                                             verbose=False)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value).startswith(pool_mod.BATCH_LIAR) and "chain" in str(e.value)
    # a grid pool, with and without the joint plan
    axes = {"v": [0, 1], "a": [0, 1, 2, 3], "b": [0, 1, 2, 3], "c": [0.5]}
    for grid, match in ((tpe.GridPool(domain, axes, joint=True), "chain"),
                        (tpe.GridPool(domain, axes), "to_pool")):
        with pytest.raises(ValueError, match=match):
            tpe.score_configs(domain, trials, grid, joint="chain")
        with pytest.raises(ValueError, match=match):
            tpe.suggest_from_pool([1], domain, trials, 0, pool=grid, joint="chain", verbose=False)
    with pytest.raises(ValueError, match="draw"):
        tpe.suggest_sampled([1], domain, trials, 0, joint="chain", draw="chain", verbose=False)
    # a context label that is not active where its group is live
    hist = tpe.collect_history(trials, pool.labels)
    bad = pool.active.copy()
    bad[0, list(domain.params).index("a")] = False
    with pytest.raises(ValueError):
        J.score_numpy(domain, hist, pool.vals, bad, tree="chain")


# -- 4. the C ABI's argument checks (no device) ------------------------------------
def test_chain_entry_checks_arguments():
    lib = L.load()
    one = ctypes.c_void_p(8)  # a non-null stand-in: validation fails before any launch
    rec = np.zeros(3, L.JOINT_LABEL_DTYPE)
    rec["kind"], rec["col"] = L.JOINT_CONT, [0, 1, 2]

    def chain(n_labels=3, n_ctx=1, n=5, ld=10, n_cols=3, list_begin=0, max_rows=10, mode=0,
              ptr=one, labels=rec.ctypes.data, tables=None):
        return lib.tpe_joint_chain_rows(labels, ptr, n_labels, n_ctx, tables, 0, ptr, n, ptr, ld,
                                        n_cols, ptr, ptr, list_begin, max_rows, None, ptr, mode,
                                        ptr, None)
    assert chain(max_rows=0) == 0 and chain(ld=0) == 0          # nothing to do
    assert chain(max_rows=0, ptr=None) == 0
    for n_ctx in (0, -1, 3, 4):
        assert chain(n_ctx=n_ctx) == -1 and b"n_ctx=%d" % n_ctx in lib.tpe_last_error()
    assert chain(n_ctx=0, max_rows=0) == -1                     # (checked before the no-op)
    assert chain(n_labels=0) == -1
    assert chain(labels=None) == -1
    assert chain(n_labels=L.COND_MAX_LABELS + 1, n_ctx=1) == L.E_UNSUPPORTED
    assert chain(n_cols=2) == -1 and b"label 2" in lib.tpe_last_error()
    assert chain(n=-1) == -1 and b"tpe_joint_chain_rows" in lib.tpe_last_error()
    assert chain(list_begin=-1) == -1
    assert chain(max_rows=-1) == -1
    assert chain(ld=-1) == -1
    for mode in (L.JOINT_OUT_ADD, 4, -1):
        assert chain(mode=mode) == -1 and b"out_mode" in lib.tpe_last_error()
    assert chain(ptr=None) == -1 and b"null pointer" in lib.tpe_last_error()
    cat = rec.copy()
    cat["kind"][1], cat["n_cat"][1] = L.JOINT_CAT, 3
    assert lib.tpe_joint_chain_rows(cat.ctypes.data, one, 3, 1, None, 9, one, 5, one, 10, 3, one,
                                    one, 0, 10, None, one, 0, one, None) == -1   # no tables
    assert lib.tpe_joint_chain_scratch_bytes(-1, 0) == -1
    assert lib.tpe_joint_chain_scratch_bytes(5, -1) == -1
    chunk = lib.tpe_joint_chunk()
    assert lib.tpe_joint_chain_scratch_bytes(7, chunk - 1) == 2 * 16 * 7
    assert lib.tpe_joint_chain_scratch_bytes(7, chunk) == 2 * 16 * 7 * 2
    assert lib.tpe_joint_chain_scratch_bytes(7, chunk) == 2 * lib.tpe_joint_scratch_bytes(7, chunk)
