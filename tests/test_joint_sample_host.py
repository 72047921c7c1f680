"""The joint draw rule on the CPU: the numpy replay of tests/joint_sample_util.py
alone (no GPU), at the seeds and cases tests/test_gpu_joint_sample.py uses.

The distribution checks hold the replay to p > 0.01 here; the GPU file holds
the device's draws of the same rows to p > 1e-4, so its inputs are ones for
which the reference alone is comfortably inside.  The stage cases' ambiguous
rows (a draw next to a bound or to a half-integer of the lattice) are counted
here from the replay alone, so the cap the GPU file applies cannot hide a
kernel error.
"""
import numpy as np
import pytest
from scipy import stats

from hyperopt_amd import Domain, hp, tpe
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from oracle import streams as S
from tests import joint_sample_util as R
from tests import joint_util as U
from tests.stream_cases import CAP64


def _chi2_p(counts, prob):
    prob = np.asarray(prob, np.float64)
    keep = prob > 0
    assert counts[~keep].sum() == 0
    return stats.chisquare(counts[keep], prob[keep] / prob[keep].sum() * counts.sum()).pvalue


# -- the cases, shared with the GPU file -----------------------------------------
def component_case():
    """41 components under a live forgetting ramp (n = 40 > LF = 25)."""
    cdf = J.sample_cdf(40, 25, 1.0)
    models = [R.model("cont", mu=0.0, sigma=1.0)]
    return models, np.zeros((1, 40)), np.asarray([0.2]), cdf


def diagonal():
    space, configs, losses = U.diagonal_case(hp)
    domain = Domain(lambda x: 0, space)
    return domain, U.make_trials(domain, configs, losses)


def one_label(kind):
    """(domain, trials) of a one-label space with 40 trials, loss = value."""
    space = {"q": hp.quniform("q", 0, 10, 3)} if kind == "quant" else \
        {"c": hp.uniform("c", 4, 7)}
    domain = Domain(lambda x: 0, space)
    rng = np.random.RandomState(5)
    if kind == "quant":
        configs = [{"q": float(3 * rng.randint(0, 4))} for _ in range(40)]
    else:
        configs = [{"c": float(rng.uniform(4, 7))} for _ in range(40)]
    return domain, U.make_trials(domain, configs, rng.uniform(size=40))


def cell_probabilities(domain, trials, rows, **kw):
    """exp(log L_below) of the pool rows ``rows`` ({label: value} dicts)."""
    pool = tpe.Pool(domain, rows)
    hist = tpe.collect_history(trials, pool.labels)
    _, lb, _ = J.score_numpy(domain, hist, pool.vals, return_parts=True, **kw)
    return np.exp(lb)


def check_components(comp, cdf, p_min):
    w = np.diff(np.concatenate([[0.0], cdf]))
    p = _chi2_p(np.bincount(comp, minlength=cdf.size), w)
    print("components: p = %.3g" % p)
    assert p > p_min


def check_diagonal(a, b, p_min):
    domain, trials = diagonal()
    prob = cell_probabilities(domain, trials, U.diagonal_pool_rows(), gamma=2.0)
    assert abs(prob.sum() - 1.0) < 1e-12
    cells = (4 * np.rint(a) + np.rint(b)).astype(np.int64)
    p = _chi2_p(np.bincount(cells, minlength=16), prob)
    print("diagonal cells: p = %.3g" % p)
    assert p > p_min


def check_lattice(q, p_min):
    domain, trials = one_label("quant")
    lattice = [0.0, 3.0, 6.0, 9.0]
    prob = cell_probabilities(domain, trials, [{"q": v} for v in lattice])
    assert abs(prob.sum() - 1.0) < 1e-12
    idx = np.rint(q / 3.0).astype(np.int64)
    assert np.array_equal(idx * 3.0, q) and idx.min() >= 0 and idx.max() <= 3
    p = _chi2_p(np.bincount(idx, minlength=4), prob)
    print("lattice: p = %.3g" % p)
    assert p > p_min


def check_ks(c, p_min):
    domain, trials = one_label("cont")
    hist = tpe.collect_history(trials, list(domain.params))
    models, mu, sig, cdf = R.below_set(domain, hist)
    assert models[0].bounded and mu.shape[1] >= 2
    assert (c >= 4.0).all() and (c < 7.0).all()
    p = stats.kstest(c, R.truncated_mixture_cdf(models[0], mu[0], sig[0], cdf)).pvalue
    print("KS: p = %.3g" % p)
    assert p > p_min


def _public_replay(domain, trials, **kw):
    hist = tpe.collect_history(trials, list(domain.params))
    return R.replay(domain, hist, R.DIST_SEED, np.arange(R.DIST_ROWS), **kw)


# -- 1. distributions of the replay ------------------------------------------------
def test_component_frequencies_follow_the_weights():
    models, mu, sig, cdf = component_case()
    comp, _ = R.replay_set(models, mu, sig, cdf, [R._key(1)], J.component_key(R.DIST_SEED), 2.0,
                           np.arange(1 << 16))
    assert comp.min() == 0 and comp.max() == 40
    check_components(comp, cdf, 0.01)


def test_diagonal_cells_follow_the_joint_below_mixture():
    domain, trials = diagonal()
    _, comp, out = _public_replay(domain, trials, gamma=2.0)
    assert comp.max() == 16  # the below set: the 16 diagonal trials, and the prior
    check_diagonal(out[0]["v"], out[1]["v"], 0.01)
    # the point of the feature: (16 x 0.4375 + 0.25) / 17 of the rows lie on the diagonal
    share = float((out[0]["v"] == out[1]["v"]).mean())
    sd = np.sqrt(0.4265 * (1 - 0.4265) / R.DIST_ROWS)
    assert abs(share - (16 * 0.4375 + 0.25) / 17) < 4 * sd
    first = float((out[0]["v"][:4096] == out[1]["v"][:4096]).mean())  # the GPU test's rows
    assert 0.39 + 0.0077 <= first <= 0.46 - 0.0077


def test_quantized_lattice_follows_the_joint_below_mixture():
    domain, trials = one_label("quant")
    _, _, out = _public_replay(domain, trials)
    check_lattice(out[0]["v"], 0.01)


def test_bounded_label_follows_the_truncated_mixture():
    domain, trials = one_label("cont")
    _, _, out = _public_replay(domain, trials)
    assert out[0]["attempts"].max() > 1 and not out[0]["clamped"].any()
    check_ks(out[0]["v"], 0.01)


# -- 2. the stage cases' ambiguous rows, from the replay alone -----------------------
_CASES = R.stage_cases()


@pytest.mark.parametrize("c", _CASES, ids=[c["name"] for c in _CASES])
def test_stage_cases_stay_within_the_ambiguity_cap(c):
    comp, out = R.replay_case(c)
    n = c["cdf"].size - 1
    assert comp.min() >= 0 and comp.max() <= n
    for m, rep in zip(c["models"], out):
        assert int(R.skipped(m, rep).sum()) <= CAP64
    if c["name"] == "bandwidth5":
        rate = 1.0 / out[0]["attempts"][comp < n].mean()
        assert 0.06 < rate < 0.10 and out[0]["attempts"].max() > 40
    if c["name"] == "clamp":
        rep = out[0]
        assert rep["clamped"].all() and (rep["attempts"] == S.MAX_ATTEMPTS).all()
        assert set(rep["v"]) == {0.0, np.nextafter(1.0, -np.inf)}
    if c["name"].startswith("smoothing"):
        rep, prior = out[0], comp == n
        assert (rep["v"][prior] != 0).all()          # never from the prior branch
        own = ~prior & (c["mu"][0][np.minimum(comp, n - 1)] == 0)
        assert own.any() and (rep["v"] == 0).sum() == (own & rep["kept"]).sum() > 0
        if c["one_plus_a"] == 1.0:
            assert rep["kept"][~prior].all()


def test_all_kinds_replay_stays_within_the_ambiguity_cap():
    from tests.test_gpu_joint import KW, N_TRIALS
    domain, trials = all_kinds_case(N_TRIALS)
    hist = tpe.collect_history(trials, list(domain.params))
    models, comp, out = R.replay(domain, hist, R.DIST_SEED, np.arange(300), **KW)
    assert len(models) == 12 and comp.max() <= 7
    for m, rep in zip(models, out):
        assert int(R.skipped(m, rep).sum()) <= CAP64, m.label


def all_kinds_case(n_trials):
    """test_gpu_joint.py's all-kinds history (same seed, same draws)."""
    from hyperopt_amd import rand
    domain = Domain(lambda x: 0, U.all_kinds_space(hp))
    rng = np.random.RandomState(17)
    configs = [rand.sample_config(domain, rng) for _ in range(n_trials)]
    losses = rng.uniform(size=n_trials)
    losses[[40, 333]] = np.inf
    return domain, U.make_trials(domain, configs, losses)


# -- 3. keys and arguments ---------------------------------------------------------
def test_component_key_is_no_label_key():
    domain = Domain(lambda x: 0, U.all_kinds_space(hp))
    for seed in (0, 1, R.DIST_SEED, 2 ** 31 - 1):
        ck = J.component_key(seed)
        assert 0 <= ck < 2 ** 64 and ck == tpe.joint_component_key(seed)
        assert ck not in set(tpe.label_keys(seed, list(domain.params)))
    assert J.component_key(0) != J.component_key(1)
    assert R.JOIN == 0x4A4F494E and R.JOIN not in (S.SAMP, S.RETR, S.PRIO, S.ANNL)


def test_draw_argument_is_checked_before_any_device_work(monkeypatch):
    domain, trials = diagonal()

    def boom(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(tpe, "engine", boom)
    monkeypatch.setattr(pool_mod, "_sample", boom)
    with pytest.raises(ValueError, match="joint=True"):
        tpe.suggest_sampled([1], domain, trials, 0, draw="joint", verbose=False)
    with pytest.raises(ValueError, match="draw="):
        tpe.suggest_sampled([1], domain, trials, 0, joint=True, draw="both", verbose=False)
    with pytest.raises(ValueError, match="draw="):
        tpe.suggest_sampled([1], domain, trials, 0, draw="", verbose=False)
