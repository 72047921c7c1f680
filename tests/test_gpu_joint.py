"""The joint Parzen criterion on the GPU (csrc/tpe_joint.hip through
tpe.score_configs(joint=True), suggest_from_pool, suggest_sampled).

Values are checked against the scalar restatement in tests/joint_util.py with
the project's fp64 log-density tolerance (test_gpu_parity.py: rtol 1e-6 per
log-density), applied as test_gpu_pool.py applies it:
|J_dev - J_ref| <= 1e-6 * (|log L_below| + |log L_above|); -inf / NaN
positions, bits across row windows and pool shapes, orders and the fold's bits
are compared exactly.
"""
import numpy as np
import pytest

from hyperopt_amd import Domain, hp, rand, tpe
from hyperopt_amd import _lib as L
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from tests import joint_util as U
from tests.test_gpu_pool import _case, _expected_order, _same_bits

pytestmark = pytest.mark.gpu

P_ROWS = 300        # no multiple of the 256-row block
N_TRIALS = 620      # gamma 0.25: 7 below, 613 above = 614 components = 2 x 256 + 102
KW = dict(prior_weight=0.7, gamma=0.25, linear_forgetting=25, bandwidth=0.25, cat_smoothing=0.5)

_SHARED = {}


def _all_kinds():
    """(domain, trials, pool, reference) of the all-kinds case, built once."""
    if not _SHARED:
        domain = Domain(lambda x: 0, U.all_kinds_space(hp))
        rng = np.random.RandomState(17)
        configs = [rand.sample_config(domain, rng) for _ in range(N_TRIALS)]
        losses = rng.uniform(size=N_TRIALS)
        losses[[40, 333]] = np.inf  # failed trials sit above
        trials = U.make_trials(domain, configs, losses)
        rows = [rand.sample_config(domain, rng) for _ in range(P_ROWS)]
        rows[5]["i"] = 2.0e6    # qnormal far tail: every component's mass is 0
        rows[299]["k"] = 0      # the pchoice option of probability zero
        rows[150]["g"] = -60.0  # a normal label 9 prior sigmas out: finite, small
        pool = tpe.Pool(domain, rows)
        ref = U.joint_reference(domain, trials, pool.vals, prior_weight=KW["prior_weight"],
                                gamma=KW["gamma"], lf=KW["linear_forgetting"],
                                bandwidth=KW["bandwidth"], cat_smoothing=KW["cat_smoothing"])
        _SHARED["case"] = (domain, trials, pool, ref)
    return _SHARED["case"]


def _fold_from(start, terms, active):
    s = start.copy()
    for j in range(terms.shape[1]):  # sequential, in domain.params order
        s = np.where(active[:, j], s + terms[:, j], s)
    return s


def _diagonal(drop=None):
    space, configs, losses = U.diagonal_case(hp)
    domain = Domain(lambda x: 0, space)
    if drop is not None:
        keep = [i for i, c in enumerate(configs) if 4 * c["a"] + c["b"] not in drop]
        configs, losses = [configs[i] for i in keep], [losses[i] for i in keep]
    return domain, U.make_trials(domain, configs, losses)


# -- 1. values -------------------------------------------------------------------
def test_values_match_scalar_restatement():
    domain, trials, pool, (ref_j, ref_b, ref_a, nb, na) = _all_kinds()
    chunk = L.load().tpe_joint_chunk()
    assert nb > 1 and (na + 1) > 2 * chunk and (na + 1) % chunk not in (0, 1)
    S, terms, Jd = tpe.score_configs(domain, trials, pool, joint=True, return_terms=True, **KW)
    assert np.isnan(terms).all()  # a flat space: every label is joint
    assert _same_bits(S, Jd)
    # log L of each set by itself (an error common to both would cancel in J)
    st = pool_mod._settings(KW["prior_weight"], KW["gamma"], KW["linear_forgetting"], True,
                            KW["bandwidth"], KW["cat_smoothing"])
    _eng, d = pool_mod._score_device(domain, trials, pool, st, False, want_parts=True)
    lb, la, j2 = d.parts[:, :P_ROWS].cpu().numpy()
    assert _same_bits(j2, Jd)
    for got, ref in ((lb, ref_b), (la, ref_a)):
        np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref))
        fin = np.isfinite(ref)
        err = np.abs(got[fin] - ref[fin])
        print("max |log L - ref| = %.3g (rel %.3g)" % (err.max(), (err / np.abs(ref[fin])).max()))
        assert (err <= 1e-6 * np.abs(ref[fin])).all()
    assert np.isneginf(ref_b[[5, 299]]).all() and np.isneginf(ref_a[[5, 299]]).all()
    np.testing.assert_array_equal(np.isnan(Jd), np.isnan(ref_j))
    np.testing.assert_array_equal(np.flatnonzero(np.isnan(Jd)), [5, 299])
    fin = ~np.isnan(ref_j)
    assert np.isfinite(ref_j[fin]).all()
    err = np.abs(Jd[fin] - ref_j[fin])
    print("max |J - J_ref| = %.3g" % err.max())
    assert (err <= 1e-6 * (np.abs(ref_b[fin]) + np.abs(ref_a[fin]))).all()
    # the numpy form of the same definition agrees too
    hist = tpe.collect_history(trials, pool.labels)
    Jn = J.score_numpy(domain, hist, pool.vals, pool.active, **KW)
    assert (np.abs(Jd[fin] - Jn[fin]) <= 1e-6 * (np.abs(ref_b[fin]) + np.abs(ref_a[fin]))).all()


# -- 2. determinism --------------------------------------------------------------
def test_bits_do_not_depend_on_pool_shape_window_or_call(monkeypatch):
    domain, trials, pool, _ = _all_kinds()
    whole = tpe.score_configs(domain, trials, pool, joint=True, **KW)
    again = tpe.score_configs(domain, trials, pool, joint=True, **KW)
    assert _same_bits(whole, again)
    sub = np.random.RandomState(2).permutation(P_ROWS)[:137]
    small = tpe.Pool.from_arrays(domain, pool.vals[sub], pool.active[sub])
    assert _same_bits(tpe.score_configs(domain, trials, small, joint=True, **KW), whole[sub])
    monkeypatch.setattr(J, "ROWS_PER_CALL", 128)  # row windows [0, 128) [128, 256) [256, 300)
    fresh = tpe.Pool.from_arrays(domain, pool.vals, pool.active)
    assert _same_bits(tpe.score_configs(domain, trials, fresh, joint=True, **KW), whole)


# -- 3. a conditional space ------------------------------------------------------
def test_conditional_space_folds_the_other_labels_onto_J():
    arrays, meta, trials, domain = _case("nested")
    labels = list(domain.params)
    rng = np.random.RandomState(11)
    pool = tpe.Pool(domain, [rand.sample_config(domain, rng) for _ in range(300)])
    kw = dict(prior_weight=meta["prior_weight"], gamma=meta["gamma"])
    S, terms, Jd = tpe.score_configs(domain, trials, pool, joint=True, return_terms=True, **kw)
    jcols = [labels.index(lab) for lab in J.joint_labels(domain)]
    assert jcols == [labels.index("root")]
    rest = np.ones(len(labels), bool)
    rest[jcols] = False
    assert np.isnan(terms[:, jcols]).all()
    np.testing.assert_array_equal(np.isnan(terms[:, rest]), ~pool.active[:, rest])
    live = pool.active & rest[None, :]
    assert _same_bits(S, _fold_from(Jd, terms, live))
    assert not _same_bits(S, Jd)
    # the conditional labels' terms are the factorised criterion's own
    S0, terms0 = tpe.score_configs(domain, trials, pool, return_terms=True, **kw)
    assert _same_bits(terms[:, rest], terms0[:, rest])
    ref = U.joint_reference(domain, trials, pool.vals, **{"prior_weight": kw["prior_weight"],
                                                          "gamma": kw["gamma"]})
    assert (np.abs(Jd - ref[0]) <= 1e-6 * (np.abs(ref[1]) + np.abs(ref[2]))).all()
    assert _same_bits(tpe.score_configs(domain, trials, pool, joint=True, **kw), S)


# -- 4. ranking ------------------------------------------------------------------
def test_suggest_from_pool_ranks_the_diagonal_first():
    domain, trials = _diagonal()
    ids = [100, 101, 102, 103]
    pool = tpe.Pool(domain, U.diagonal_pool_rows())
    docs = tpe.suggest_from_pool(ids, domain, trials, 0, pool=pool, gamma=2.0, joint=True,
                                 verbose=False)
    assert len(docs) == 4
    assert {pool.row_of[i] for i in ids} == {0, 5, 10, 15}
    for doc in docs:
        assert doc["misc"]["vals"]["a"] == doc["misc"]["vals"]["b"]
    S = tpe.score_configs(domain, trials, pool, gamma=2.0, joint=True)
    assert [pool.row_of[i] for i in ids] == _expected_order(S, np.zeros(16), 4).tolist()
    # the taken rule: the next four are the best of the rest
    more = [104, 105, 106, 107]
    tpe.suggest_from_pool(more, domain, trials, 0, pool=pool, gamma=2.0, joint=True,
                          verbose=False)
    taken = np.zeros(16)
    taken[[0, 5, 10, 15]] = 1
    assert [pool.row_of[i] for i in more] == _expected_order(S, taken, 4).tolist()
    # the factorised criterion is flat here and does not find the diagonal
    flat = tpe.Pool(domain, U.diagonal_pool_rows())
    tpe.suggest_from_pool(ids, domain, trials, 0, pool=flat, gamma=2.0, verbose=False)
    assert {flat.row_of[i] for i in ids} != {0, 5, 10, 15}


def test_suggest_from_pool_distinct_with_joint():
    ids = [100, 101, 102, 103]
    twice = U.diagonal_pool_rows() + U.diagonal_pool_rows()
    domain, trials = _diagonal()
    pool = tpe.Pool(domain, twice)
    # every configuration is in the history: nothing is fresh
    assert tpe.suggest_from_pool(ids, domain, trials, 0, pool=pool, gamma=2.0, joint=True,
                                 distinct=True, verbose=False) == []
    # a history without configurations 5 and 10: only their first rows are fresh
    domain, trials = _diagonal(drop={5, 10})
    pool = tpe.Pool(domain, twice)
    docs = tpe.suggest_from_pool(ids, domain, trials, 0, pool=pool, gamma=2.0, joint=True,
                                 distinct=True, verbose=False)
    assert len(docs) == 2 and sorted(pool.row_of.values()) == [5, 10]
    S = tpe.score_configs(domain, trials, pool, gamma=2.0, joint=True)
    stale = np.ones(32)
    stale[[5, 10]] = 0
    assert [pool.row_of[i] for i in ids[:2]] == _expected_order(S, stale, 2).tolist()


# -- 5. suggest_sampled ----------------------------------------------------------
def test_suggest_sampled_ranks_the_sampled_pool_by_the_joint_score():
    domain, trials, _, _ = _all_kinds()
    labels = list(domain.params)
    seed, n, ids = 123, 256, [700, 701, 702, 703, 704]
    kw = {k: KW[k] for k in ("prior_weight", "gamma", "linear_forgetting")}
    docs = tpe.suggest_sampled(ids, domain, trials, seed, n_EI_candidates=n, joint=True,
                               bandwidth=KW["bandwidth"], cat_smoothing=KW["cat_smoothing"],
                               verbose=False, **kw)
    pool = tpe.Pool.sample(domain, trials, seed, n, **kw)
    born = pool.scores().copy()
    S = tpe.score_configs(domain, trials, pool, joint=True, **KW)
    order = _expected_order(S, np.zeros(n), len(ids))
    assert order.tolist() != _expected_order(born, np.zeros(n), len(ids)).tolist()
    assert len(docs) == len(ids)
    for doc, r in zip(docs, order):
        cfg = pool.config(int(r))
        assert {lab: doc["misc"]["vals"][lab][0] for lab in labels} == cfg


# -- 6. startup and errors -------------------------------------------------------
def test_startup_phase_is_unchanged():
    domain, trials = _diagonal()
    ids = [100, 101, 102]
    a, b = tpe.Pool(domain, U.diagonal_pool_rows()), tpe.Pool(domain, U.diagonal_pool_rows())
    kw = dict(n_startup_jobs=65, gamma=2.0, verbose=False)  # (64 trials: still starting up)
    tpe.suggest_from_pool(ids, domain, trials, 9, pool=a, joint=True, **kw)
    tpe.suggest_from_pool(ids, domain, trials, 9, pool=b, **kw)
    assert [a.row_of[i] for i in ids] == [b.row_of[i] for i in ids] == \
        pool_mod.startup_rows(tpe.Pool(domain, U.diagonal_pool_rows()), 9, 3).tolist()
    d1 = tpe.suggest_sampled(ids, domain, trials, 9, n_EI_candidates=64, n_startup_jobs=65,
                             joint=True, verbose=False)
    d2 = tpe.suggest_sampled(ids, domain, trials, 9, n_EI_candidates=64, n_startup_jobs=65,
                             verbose=False)
    assert [d["misc"]["vals"] for d in d1] == [d["misc"]["vals"] for d in d2]


def test_grid_pool_and_label_free_space_raise():
    domain, trials = _diagonal()
    grid = tpe.GridPool(domain, {"a": [0, 1, 2, 3], "b": [0, 1, 2, 3]})
    with pytest.raises(ValueError, match="to_pool"):
        tpe.score_configs(domain, trials, grid, joint=True)
    with pytest.raises(ValueError, match="to_pool"):
        tpe.suggest_from_pool([1], domain, trials, 0, pool=grid, joint=True, verbose=False)
    S = tpe.score_configs(domain, trials, grid.to_pool(), gamma=2.0, joint=True)
    assert set(_expected_order(S, np.zeros(16), 4).tolist()) == {0, 5, 10, 15}
    empty = Domain(lambda x: 0, {"x": 1.0})
    none = U.make_trials(empty, [{}] * 3, [0.1, 0.2, 0.3])
    pool = tpe.Pool.from_arrays(empty, np.zeros((2, 0)), np.zeros((2, 0), bool))
    with pytest.raises(ValueError, match="joint"):
        tpe.score_configs(empty, none, pool, joint=True)
    with pytest.raises(ValueError, match="joint"):
        tpe.suggest_sampled([1], empty, none, 0, n_startup_jobs=0, joint=True, verbose=False)


def test_limits_are_unsupported_and_bad_arguments_are_refused():
    lib = L.load()
    rec = np.zeros(L.COND_MAX_LABELS + 1, L.JOINT_LABEL_DTYPE)
    rec["kind"], rec["prior_sigma"], rec["prior_r"] = L.JOINT_CONT, 1.0, 1.0
    host = rec.ctypes.data
    args = (None, 0, None, 0, None, 1024, 1024, 0, 16, None, None, None, None)
    assert lib.tpe_joint_score(host, None, L.COND_MAX_LABELS + 1, *args) == L.E_UNSUPPORTED
    assert lib.tpe_joint_prep(host, None, L.COND_MAX_LABELS + 1, None, None, 16, 1024, None, 4,
                              None, None) == L.E_UNSUPPORTED
    cat = np.zeros(1, L.JOINT_LABEL_DTYPE)
    cat["kind"], cat["n_cat"] = L.JOINT_CAT, L.JOINT_MAX_CAT + 1
    assert lib.tpe_joint_score(cat.ctypes.data, None, 1, *args) == L.E_UNSUPPORTED
    cat["n_cat"] = 4  # fits, but its tables do not: refused before any launch
    assert lib.tpe_joint_score(cat.ctypes.data, None, 1, *args) == -1
    assert lib.tpe_joint_score(host, None, 0, *args) == -1            # no label
    assert lib.tpe_joint_score(host, None, 1, *args) == -1            # null pointers
    rec["col"][0] = 4096                                              # a column the pool lacks
    assert lib.tpe_joint_score(host, None, 1, *args) == -1
    assert lib.tpe_joint_scratch_bytes(-1, 4) == -1 and lib.tpe_joint_set_doubles(-1, 4) == -1
    chunk = lib.tpe_joint_chunk()
    assert lib.tpe_joint_scratch_bytes(10, chunk - 1) == 16 * 10
    assert lib.tpe_joint_scratch_bytes(10, chunk) == 16 * 10 * 2
    assert b"tpe_joint" in lib.tpe_last_error()


# -- 7. a set without rows ---------------------------------------------------------
@pytest.mark.parametrize("name", ["empty", "one", "foreign_below"])
def test_a_set_without_rows_is_the_prior_alone(name, monkeypatch):
    """No trial, one trial (no above row) and a below set emptied by a foreign
    row, on pool rows whose fit coordinate is exactly 0 (x == 0.0, x == 1.0 on
    a log kind): the places of a pass past the last component must count for
    nothing, whatever their arithmetic gives."""
    domain = Domain(lambda x: 0, U.zero_coordinate_space(hp))
    configs, losses = U.small_histories()[name]
    trials = U.make_trials(domain, configs, losses)
    pool = tpe.Pool(domain, U.zero_coordinate_rows())
    P = len(pool)
    ref_j, ref_b, ref_a, nb, na = U.joint_reference(domain, trials, pool.vals)
    assert (nb, na) == {"empty": (0, 0), "one": (1, 0), "foreign_below": (0, 2)}[name]
    assert np.isfinite(ref_j).all()
    st = pool_mod._settings(1.0, 0.25, 25, True, J.BANDWIDTH, J.CAT_SMOOTHING)
    make = pool_mod._parts  # (NaN wherever the scoring writes nothing)
    monkeypatch.setattr(pool_mod, "_parts", lambda *a: make(*a).fill_(float("nan")))
    _eng, d = pool_mod._score_device(domain, trials, pool, st, False, want_parts=True)
    lb, la, jd = d.parts[:, :P].cpu().numpy()
    for got, ref in ((lb, ref_b), (la, ref_a)):
        print(name, "max |log L - ref| = %.3g" % np.abs(got - ref).max())
        assert (np.abs(got - ref) <= 1e-6 * np.abs(ref)).all()
    assert (np.abs(jd - ref_j) <= 1e-6 * (np.abs(ref_b) + np.abs(ref_a))).all()
    S = tpe.score_configs(domain, trials, pool, joint=True)
    assert _same_bits(S, jd)
    if name == "empty":  # both sets are the prior: J is exactly 0
        assert (S == 0.0).all()
