"""``joint="chain"`` on the GPU, through the public functions: every group of
labels conditioned on its context by the chain rule (hyperopt_amd/joint.py
"Chains", csrc/tpe_joint_chain.hip).

Values are checked against the scalar restatement of tests/joint_chain_util.py:
|got - ref| <= 1e-6 * sum over the row's live groups of (|log L_below| + |log
L_above|, plus the two context marginals' |.| for a group with a context), the
project's fp64 log-density rule as tests/joint_tree_util.py applies it.  -inf /
NaN positions, orders and every "same bits" statement are exact.
"""
import numpy as np
import pytest

from hyperopt_amd import Domain, rand, tpe
from hyperopt_amd import joint as J
from tests import joint_chain_util as CU
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
        ref = CU.chain_reference(domain, trials, pool.vals, pool.active, **kw)
        _SHARED["nested"] = (domain, trials, pool, kw, ref)
    return _SHARED["nested"]


def _two_clause():
    if "two" not in _SHARED:
        domain = Domain(lambda x: 0, TU.two_clause_space())
        rng = np.random.RandomState(7)
        configs = [rand.sample_config(domain, rng) for _ in range(120)]
        trials = U.make_trials(domain, configs, rng.uniform(size=120))
        pool = tpe.Pool(domain, [rand.sample_config(domain, rng) for _ in range(60)])
        ref = CU.chain_reference(domain, trials, pool.vals, pool.active)
        _SHARED["two"] = (domain, trials, pool, {}, ref)
    return _SHARED["two"]


def _check_values(domain, trials, pool, kw, ref):
    S, terms, Cm = tpe.score_configs(domain, trials, pool, joint="chain", return_terms=True, **kw)
    rS, rC = ref[0], ref[1]
    live = TU.group_live(domain, pool.active)
    assert Cm.shape == rC.shape and np.isnan(terms).all() and terms.shape == pool.vals.shape
    assert not np.isnan(rC[live]).any()
    np.testing.assert_array_equal(np.isnan(Cm), ~live)       # NaN exactly where not live
    assert _same_bits(S, TU.fold_live(Cm, live))             # S is the fold of C's columns
    err = np.abs(S - rS)
    tol = CU.tolerance(*ref[2:6])
    print("max |S - S_ref| = %.3g (tolerance there %.3g)" % (err.max(), tol[err.argmax()]))
    assert (err <= tol).all()
    for g in range(Cm.shape[1]):
        on = live[:, g]
        assert (np.abs(Cm[on, g] - rC[on, g]) <= CU.column_tolerance(ref, g)[on]).all()
    assert _same_bits(tpe.score_configs(domain, trials, pool, joint="chain", **kw), S)
    # the root column is joint=True's J
    _, _, Jroot = tpe.score_configs(domain, trials, pool, joint=True, return_terms=True, **kw)
    assert _same_bits(Cm[:, 0], Jroot)
    # and the numpy form agrees
    hist = tpe.collect_history(trials, pool.labels)
    Sn = J.score_numpy(domain, hist, pool.vals, pool.active, tree="chain", **kw)
    assert (np.abs(S - Sn) <= tol).all()
    return S, Cm


# -- 1. values -------------------------------------------------------------------
def test_values_on_the_nested_case():
    domain, trials, pool, kw, ref = _nested()
    contexts = J.joint_contexts(domain)
    assert [bool(c) for c in contexts] == [False, False, False, True, True, False]
    S, Cm = _check_values(domain, trials, pool, kw, ref)
    # "chain" is neither True nor "tree": the groups with a context differ
    _, _, Jm = tpe.score_configs(domain, trials, pool, joint="tree", return_terms=True, **kw)
    live = TU.group_live(domain, pool.active)
    for g, ctx in enumerate(contexts):
        on = live[:, g]
        assert on.any()
        assert _same_bits(Cm[on, g], Jm[on, g]) == (not ctx)  # empty context: C_g is J_g
    assert not _same_bits(S, tpe.score_configs(domain, trials, pool, joint=True, **kw))


def test_values_on_the_two_clause_space():
    domain, trials, pool, kw, ref = _two_clause()
    assert all(J.joint_contexts(domain)[1:])                  # every group has a context
    _check_values(domain, trials, pool, kw, ref)


# -- 2. same bits ----------------------------------------------------------------
def test_flat_space_has_the_bits_of_joint_true():
    from tests.test_gpu_joint import KW, _all_kinds
    domain, trials, pool, _ = _all_kinds()
    plain = tpe.score_configs(domain, trials, pool, joint=True, **KW)
    S, terms, Cm = tpe.score_configs(domain, trials, pool, joint="chain", return_terms=True, **KW)
    assert _same_bits(S, plain) and np.isnan(terms).all()
    assert Cm.shape == (len(pool), 1) and _same_bits(Cm[:, 0], plain)


def test_empty_contexts_have_the_bits_of_tree():
    domain, trials = TU.branch_diagonal_case()
    pool = tpe.Pool(domain, TU.branch_pool_rows())
    kw = dict(gamma=TU.GAMMA_DIAGONAL)
    assert J.joint_contexts(domain) == [[], [], []]
    St, _, Jm = tpe.score_configs(domain, trials, pool, joint="tree", return_terms=True, **kw)
    Sc, _, Cm = tpe.score_configs(domain, trials, pool, joint="chain", return_terms=True, **kw)
    assert _same_bits(Sc, St) and _same_bits(Cm, Jm)


# -- 3. the cross-level case -----------------------------------------------------
def test_suggest_from_pool_finds_the_root_and_branch_pairs():
    """A root label that is good only together with a label inside a branch:
    the chain criterion hands out the diagonal a == b; ``joint="tree"`` (two
    independent mixtures) and ``joint=True`` (a alone) do not."""
    domain, trials = CU.cross_level_case()
    rows = CU.cross_pool_rows()
    kw = dict(gamma=TU.GAMMA_DIAGONAL, verbose=False)
    ids = [100, 101, 102, 103]
    pool = tpe.Pool(domain, rows)
    docs = tpe.suggest_from_pool(ids, domain, trials, 0, pool=pool, joint="chain", **kw)
    assert len(docs) == 4 and {pool.row_of[i] for i in ids} == set(CU.DIAGONAL)
    for doc in docs:
        assert doc["misc"]["vals"]["a"] == doc["misc"]["vals"]["b"]
        assert doc["misc"]["vals"]["v"] == [0] and doc["misc"]["vals"]["c"] == []
    S = tpe.score_configs(domain, trials, pool, gamma=TU.GAMMA_DIAGONAL, joint="chain")
    assert [pool.row_of[i] for i in ids] == _expected_order(S, np.zeros(17), 4).tolist()
    ref = CU.chain_reference(domain, trials, pool.vals, pool.active, gamma=TU.GAMMA_DIAGONAL)
    assert (np.abs(S - ref[0]) <= CU.tolerance(*ref[2:6])).all()
    assert np.sort(S)[-4] - np.sort(S)[-5] > 0.5              # a wide gap to the fifth row
    for other in ("tree", True):
        p = tpe.Pool(domain, rows)
        tpe.suggest_from_pool(ids, domain, trials, 0, pool=p, joint=other, **kw)
        assert {p.row_of[i] for i in ids} != set(CU.DIAGONAL)


# -- 4. invariance ---------------------------------------------------------------
def test_bits_do_not_depend_on_pool_shape_window_or_call(monkeypatch):
    domain, trials, pool, kw, _ = _nested()
    whole = tpe.score_configs(domain, trials, pool, joint="chain", **kw)
    assert _same_bits(tpe.score_configs(domain, trials, pool, joint="chain", **kw), whole)
    sub = np.random.RandomState(2).permutation(len(pool))[:137]
    small = tpe.Pool.from_arrays(domain, pool.vals[sub], pool.active[sub])
    assert _same_bits(tpe.score_configs(domain, trials, small, joint="chain", **kw), whole[sub])
    monkeypatch.setattr(J, "ROWS_PER_CALL", 128)  # list windows [0, 128) [128, 256) [256, 300)
    fresh = tpe.Pool.from_arrays(domain, pool.vals, pool.active)
    S, _, Cm = tpe.score_configs(domain, trials, fresh, joint="chain", return_terms=True, **kw)
    assert _same_bits(S, whole)
    assert _same_bits(S, TU.fold_live(Cm, TU.group_live(domain, pool.active)))


# -- 5. edges --------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CU.rooted_edge_histories()))
def test_edge_histories(name):
    """A branch never tried, tried above only, a foreign trial with half a
    group's labels, no trial at all, and a foreign trial that lacks the
    context label: dropped from that group's sets, n shrinks."""
    domain = Domain(lambda x: 0, CU.rooted_branch_space())
    configs, losses = CU.rooted_edge_histories()[name]
    trials = U.make_trials(domain, configs, losses)
    pool = tpe.Pool(domain, CU.rooted_pool_rows())
    assert J.joint_contexts(domain)[1:] == [["r"], ["r"]]
    ref = CU.chain_reference(domain, trials, pool.vals, pool.active)
    ab = [g.labels for g in J.joint_groups(domain)].index(["a", "b"])
    assert ref[6][ab] == {"never_tried": (0, 0), "above_only": (0, 4), "foreign_half": (0, 4),
                          "empty": (0, 0), "foreign_context": (0, 4)}[name]
    S, Cm = _check_values(domain, trials, pool, {}, ref)
    if name in ("never_tried", "empty"):
        # both sets are the prior alone: full and marginal differ by the same
        # prior factors on either side, and C_g is exactly 0
        assert (Cm[:16, ab] == 0.0).all()
    if name == "empty":
        assert (S == 0.0).all()
    if name == "foreign_context":  # the trial without r changes nothing in (a, b)'s term ...
        base = U.make_trials(domain, configs[:-1], losses[:-1])
        _, _, C0 = tpe.score_configs(domain, base, pool, joint="chain", return_terms=True)
        assert _same_bits(Cm[:, ab], C0[:, ab])
        # ... though "tree", whose sets need (a, b) alone, counts it
        _, _, J1 = tpe.score_configs(domain, trials, pool, joint="tree", return_terms=True)
        _, _, J0 = tpe.score_configs(domain, base, pool, joint="tree", return_terms=True)
        assert not _same_bits(J1[:, ab], J0[:, ab])


# -- 6. sampling -----------------------------------------------------------------
def test_pool_sample_chain():
    domain, trials, _pool, kw, _ = _nested()
    n = 300
    pool = tpe.Pool.sample(domain, trials, SEED, n, joint="chain", keep_terms=True, **kw)
    tree = tpe.Pool.sample(domain, trials, SEED, n, joint="tree", **kw)
    assert isinstance(pool, tpe.SampledPool) and len(pool) == n
    dv = pool._born().vals[:, :n].cpu().numpy()
    assert _same_bits(dv, tree._born().vals[:, :n].cpu().numpy())      # the rows of "tree"
    np.testing.assert_array_equal(pool.active, tree.active)
    assert np.isnan(pool.terms()).all()
    born = pool.scores().copy()
    rows = tpe.Pool.from_arrays(domain, pool.vals, pool.active)         # materialised
    S = tpe.score_configs(domain, trials, rows, joint="chain", **kw)
    assert _same_bits(born, S)
    assert not _same_bits(born, tree.scores())
    ref = CU.chain_reference(domain, trials, pool.vals, pool.active, **kw)
    assert (np.abs(born - ref[0]) <= CU.tolerance(*ref[2:6])).all()


def _doc_config(doc):
    return {k: v[0] for k, v in doc["misc"]["vals"].items() if v}


def test_suggest_sampled_chain():
    domain, trials = CU.cross_level_case()
    ids = [200, 201, 202, 203, 204]
    kw = dict(n_EI_candidates=256, gamma=TU.GAMMA_DIAGONAL, verbose=False)
    # draw="joint": the k best rows of Pool.sample(joint="chain") by its born S
    docs = tpe.suggest_sampled(ids, domain, trials, SEED, joint="chain", draw="joint", **kw)
    pool = tpe.Pool.sample(domain, trials, SEED, 256, joint="chain", gamma=TU.GAMMA_DIAGONAL)
    rows = _expected_order(pool.scores(), np.zeros(256), len(ids))
    assert [d["tid"] for d in docs] == ids
    assert [_doc_config(d) for d in docs] == [pool.config(int(r)) for r in rows]
    # the default draw samples blind and ranks by the chain S
    docs = tpe.suggest_sampled(ids, domain, trials, SEED, joint="chain", **kw)
    plain = tpe.Pool.sample(domain, trials, SEED, 256, gamma=TU.GAMMA_DIAGONAL)
    S = tpe.score_configs(domain, trials, plain, joint="chain", gamma=TU.GAMMA_DIAGONAL)
    rows = _expected_order(S, np.zeros(256), len(ids))
    assert [_doc_config(d) for d in docs] == [plain.config(int(r)) for r in rows]
    # distinct, under both draws: valid documents, pairwise distinct, not in the history
    labels = list(domain.params)
    hist = tpe.collect_history(trials, labels)

    def key(vals, active):  # (None where the label is not live: NaN never equals itself)
        return tuple(float(v) if on else None for v, on in zip(vals, active))
    seen = {key(hist.vals[t], hist.active[t]) for t in range(hist.tids.size)}
    for draw in ("joint", "factorised"):
        fresh = tpe.suggest_sampled(ids, domain, trials, SEED, joint="chain", draw=draw,
                                    distinct=True, **kw)
        cfgs = [_doc_config(d) for d in fresh]
        assert len(cfgs) == len(ids)
        assert len({tuple(sorted(c.items())) for c in cfgs}) == len(cfgs)
        made = tpe.Pool(domain, cfgs)                          # valid configurations
        for r in range(len(cfgs)):
            assert key(made.vals[r], made.active[r]) not in seen
