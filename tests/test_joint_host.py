"""The joint Parzen criterion on the host: ``joint.score_numpy`` against the
scalar restatement (tests/joint_util.py), the joint-label set, the mixture
weights, foreign rows and the interaction case the criterion is for.

Tolerance: both sides are fp64 evaluations of the same formulas that differ
only in who rounds (numpy's vector log / exp against libm's): a log L is a
log-sum-exp over at most 62 x 12 factors of magnitude ~10, so 1e-10 relative
to |log L| is four orders above the rounding and far below any modelling
difference.
"""
import numpy as np
import pytest

from hyperopt_amd import Domain, hp, rand, tpe
from hyperopt_amd import joint as J
from oracle import tpe_oracle as O
from tests import joint_util as U
from tests.golden import spaces


def _domain(space):
    return Domain(lambda x: 0, space)


def test_score_numpy_matches_scalar_restatement_all_kinds():
    domain = _domain(U.all_kinds_space(hp))
    labels = list(domain.params)
    rng = np.random.RandomState(3)
    configs = [rand.sample_config(domain, rng) for _ in range(60)]
    losses = rng.uniform(size=60)
    losses[7] = np.inf  # a failed trial sits above
    trials = U.make_trials(domain, configs, losses)
    rows = [rand.sample_config(domain, rng) for _ in range(40)]
    rows[5]["i"] = 2.0e6   # qnormal far tail: no mass under any component
    rows[9]["k"] = 0       # the pchoice option of probability zero
    pool_vals = np.asarray([[float(c[lab]) for lab in labels] for c in rows])
    kw = dict(prior_weight=0.7, gamma=0.3, bandwidth=0.25, cat_smoothing=0.5)
    ref_j, ref_b, ref_a, nb, na = U.joint_reference(domain, trials, pool_vals, lf=25, **kw)
    assert nb > 1 and nb + na == 60
    hist = tpe.collect_history(trials, labels)
    got_j, got_b, got_a = J.score_numpy(domain, hist, pool_vals, linear_forgetting=25,
                                        return_parts=True, **kw)
    for got, ref in ((got_b, ref_b), (got_a, ref_a)):
        np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref))
        fin = np.isfinite(ref)
        assert fin.sum() == 38
        assert (np.abs(got[fin] - ref[fin]) <= 1e-10 * np.abs(ref[fin])).all()
    np.testing.assert_array_equal(np.isnan(got_j), np.isnan(ref_j))
    assert np.isnan(ref_j[[5, 9]]).all() and np.isnan(ref_j).sum() == 2
    fin = ~np.isnan(ref_j)
    assert (np.abs(got_j[fin] - ref_j[fin]) <= 1e-10 * (np.abs(ref_b[fin]) +
                                                        np.abs(ref_a[fin]))).all()


def test_joint_label_sets():
    flat = _domain(U.all_kinds_space(hp))
    assert J.joint_labels(flat) == list(flat.params)
    nested = _domain(spaces.nested(hp))
    assert J.joint_labels(nested) == ["root"]
    assert J.joint_labels(_domain(spaces.readme(hp))) == ["a"]
    mixed = _domain({"x": hp.uniform("x", 0, 1),
                     "c": hp.choice("c", [hp.normal("y", 0, 1), hp.quniform("z", 0, 4, 1)])})
    assert J.joint_labels(mixed) == [lab for lab in mixed.params if lab in ("x", "c")]
    empty = _domain({"x": 1.0})
    assert J.joint_labels(empty) == []
    with pytest.raises(ValueError):
        J.label_models(empty)
    with pytest.raises(ValueError):
        J.score_numpy(empty, tpe.collect_history(U.make_trials(empty, [], []), []),
                      np.zeros((1, 0)))


@pytest.mark.parametrize("n", [0, 1, 24, 25, 26, 40])
@pytest.mark.parametrize("pw", [1.0, 0.3])
def test_log_weights(n, pw):
    lf = 25
    v = O.linear_forgetting_weights(n, lf)
    if n < lf:
        assert (v == 1.0).all()
    else:
        assert (v[n - lf:] == 1.0).all() and (n == lf or v[0] == 1.0 / n)
    want = np.log(np.concatenate([v, [pw]]) / (v.sum() + pw))
    got = J.log_weights(n, lf, pw)
    assert got.shape == (n + 1,)
    np.testing.assert_array_equal(got, want)
    assert abs(np.exp(got).sum() - 1.0) < 1e-12


def test_foreign_rows_are_dropped():
    space = {"a": hp.choice("a", [0, 1, 2]), "x": hp.uniform("x", 0, 1),
             "q": hp.quniform("q", 0, 8, 2)}
    domain = _domain(space)
    labels = list(domain.params)
    rng = np.random.RandomState(5)
    configs = [rand.sample_config(domain, rng) for _ in range(30)]
    losses = rng.uniform(size=30)
    foreign = [2, 3, 11, 29]
    losses[3] = 0.0  # a foreign row inside the below set
    for r in foreign:
        del configs[r]["x"]
    trials = U.make_trials(domain, configs, losses)
    hist = tpe.collect_history(trials, labels)
    isb, isa = tpe.split_masks(hist, 0.5)
    cols = [labels.index(lab) for lab in J.joint_labels(domain)]
    rows_b, rows_a = J.set_rows(hist, isb, cols), J.set_rows(hist, isa, cols)
    assert isb[3] and 3 not in rows_b
    assert not set(foreign) & (set(rows_b.tolist()) | set(rows_a.tolist()))
    assert rows_b.size + rows_a.size == 30 - len(foreign)
    assert rows_b.size == isb.sum() - 1  # (the split is decided before the rows are dropped)
    pool_vals = np.asarray([[float(c[lab]) for lab in labels]
                            for c in (rand.sample_config(domain, rng) for _ in range(12))])
    ref = U.joint_reference(domain, trials, pool_vals, gamma=0.5)
    assert (ref[3], ref[4]) == (rows_b.size, rows_a.size)
    got = J.score_numpy(domain, hist, pool_vals, gamma=0.5, return_parts=True)
    for g, r in zip(got[1:], ref[1:3]):
        assert (np.abs(g - r) <= 1e-10 * np.abs(r)).all()


def test_diagonal_case_ranks_the_diagonal_first():
    space, configs, losses = U.diagonal_case(hp)
    domain = _domain(space)
    trials = U.make_trials(domain, configs, losses)
    pool = tpe.Pool(domain, U.diagonal_pool_rows())
    hist = tpe.collect_history(trials, pool.labels)
    isb, _ = tpe.split_masks(hist, 2.0)
    assert isb.sum() == 16 and all(configs[r]["a"] == configs[r]["b"]
                                   for r in np.flatnonzero(isb))
    score = J.score_numpy(domain, hist, pool.vals, pool.active, gamma=2.0)
    assert set(np.argsort(-score, kind="stable")[:4].tolist()) == {0, 5, 10, 15}
    diag = np.zeros(16, bool)
    diag[[0, 5, 10, 15]] = True
    assert score[diag].min() >= 0.77 and score[~diag].max() <= -0.07
    ref = U.joint_reference(domain, trials, pool.vals, gamma=2.0)[0]
    assert (np.abs(score - ref) <= 1e-10 * 20).all()


@pytest.mark.parametrize("name", ["empty", "one", "foreign_below"])
def test_a_set_without_rows_is_the_prior_alone(name):
    domain = _domain(U.zero_coordinate_space(hp))
    configs, losses = U.small_histories()[name]
    trials = U.make_trials(domain, configs, losses)
    pool = tpe.Pool(domain, U.zero_coordinate_rows())
    ref_j, ref_b, ref_a, nb, na = U.joint_reference(domain, trials, pool.vals)
    assert (nb, na) == {"empty": (0, 0), "one": (1, 0), "foreign_below": (0, 2)}[name]
    assert np.isfinite(ref_j).all()
    hist = tpe.collect_history(trials, pool.labels)
    got = J.score_numpy(domain, hist, pool.vals, pool.active, return_parts=True)
    for g, r in zip(got[1:], (ref_b, ref_a)):
        assert (np.abs(g - r) <= 1e-10 * np.abs(r)).all()
    if name == "empty":  # both sets are the prior: J is exactly 0
        assert (got[0] == 0.0).all() and (ref_j == 0.0).all()
