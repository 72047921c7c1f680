"""The scale cases (tests/scale_cases.py) are sound, shown with the oracle
alone: a power-of-two image has the scaled canonical fit bit for bit, every
image's scores agree with its yardstick's, the tiny cases reach the EPS
floors, and the oracle's own sampler passes the distribution check that
tests/test_gpu_scales.py applies to the fp32 stream -- at the same size and
threshold, so a failure there is the device's.
"""
import numpy as np
import pytest
from scipy import stats

from oracle import tpe_oracle as O
from tests import scale_cases as SC


def test_case_table():
    assert len(set(SC.IDS)) == len(SC.CASES) == 27
    assert len({c.key for c in SC.CASES}) == len(SC.CASES)
    for c in SC.CASES:
        assert c.cand.size == SC.N_INJ and c.above.size == SC.T - 14
        assert c.below.size == (25 if c.group == "outward" else 14)
        assert np.all(np.isfinite(c.cand)) and np.all(np.isfinite(c.above))
        if c.kind.startswith("q"):
            assert np.all(SC.on_lattice(c, c.cand)) and np.all(SC.on_lattice(c, c.above))
    # the outward cases are what they are named for
    # (fp32 rounds 0.7 below itself -- outward; 1.3 also down, which only
    # costs the stream its last value below `high`)
    assert float(np.float32(0.7)) < 0.7 and float(np.float32(1.3)) < 1.3
    lo, hi = SC.case("loguniform(0.7,1.3)").args
    print("log twin: (float)low - low = %.3g, (float)high - high = %.3g"
          % (float(np.float32(lo)) - lo, float(np.float32(hi)) - hi))
    assert float(np.float32(lo)) != lo and float(np.float32(hi)) != hi


def test_bound32_is_the_smallest_float_not_below():
    """oracle/streams.py bound32 (the replay of tpe_sample.hpp's): the fp32
    comparisons lo <= y and y < hi then decide as the fp64 bounds do."""
    from oracle.streams import bound32
    lo, hi = SC.case("loguniform(0.7,1.3)").args
    for b in (0.7, 1.3, -0.7, -1.3, lo, hi, 1e6 + 1 / 3, 1e-30, -1e-30):
        f = bound32(b)
        assert f == float(np.float32(f)) and f >= b
        assert float(np.nextafter(np.float32(f), np.float32(-np.inf))) < b
    for b in (-5.0, 0.0, 5.0, 1000.0, 1010.0, 1e6, 1e6 + 1, 2.0 ** -20, np.inf, -np.inf):
        assert bound32(b) == b  # exact in fp32: untouched


def test_fp32_resolution_rule():
    """posterior_params' draw32 (DESIGN.md "Scale and offset"): only
    uniform(1e6, 1e6 + 1) leaves the fp32 stream; the cases the issue keeps on
    the table path, and the suite's and the benchmark's spaces, stay."""
    from hyperopt_amd.engine import DRAW32_MIN_STEPS, posterior_params
    for c in SC.CONT:
        if c.group != "tiny":
            assert posterior_params(c.kind, c.args)["draw32"] == (c.path != "fp64"), c.name
    for kind, args in (("uniform", (-5.0, 5.0)), ("loguniform", (-5.0, 0.0)),
                       ("normal", (0.0, 2.0)), ("lognormal", (0.0, 1.0)),
                       ("loguniform", (-7.0, 0.0)), ("uniform", (-10.0, 10.0)),
                       ("normal", (0.0, 1.0)), ("uniform", (0.0, 1.0))):
        assert posterior_params(kind, args)["draw32"]
    # the threshold itself: fp32 spacing at the far end against prior_sigma
    for e, want in ((16, True), (17, True), (18, False), (19, False)):
        far = 2.0 ** e + 10.0
        P = posterior_params("uniform", (2.0 ** e, far))
        assert P["draw32"] == want
        assert want == (float(np.spacing(np.float32(far))) * DRAW32_MIN_STEPS <= 10.0)


@pytest.mark.parametrize("c", SC.POW2 + [SC.case("normal(0,2)*2^-40")], ids=lambda c: c.name)
def test_pow2_fit_is_the_scaled_canonical_fit(c):
    """adaptive_parzen_normal of observations times 2^k: weights equal, means
    and bandwidths times 2^k, bit for bit (n = 14 and 2986; 0, 1, 25 and 3000
    below)."""
    s = 2.0 ** c.k
    canon = SC.case(c.canon)
    for (w, mu, sg), (w0, mu0, sg0) in zip(SC.fits(c), SC.fits(canon)):
        assert np.array_equal(w, w0) and np.array_equal(mu, mu0 * s)
        assert np.array_equal(sg, sg0 * s)
    fam, pmu, psig, tf, _, _, _ = SC.spec(canon)
    obs = np.concatenate([canon.below, canon.above])
    for n in (0, 1, 25, 3000):
        w0, mu0, sg0 = O.adaptive_parzen_normal(obs[:n], 1.0, pmu, psig)
        w, mu, sg = O.adaptive_parzen_normal(obs[:n] * s, 1.0, pmu * s, psig * s)
        assert np.array_equal(w, w0) and np.array_equal(mu, mu0 * s)
        assert np.array_equal(sg, sg0 * s)


# what the oracle may disagree with itself by, per group: fp64 rounding of a
# score of magnitude <= ~50 whose terms (x - mu) / sigma lose log2(|x| / sigma)
# bits to the offset -- 2^-52 * 50 * |x| / sigma_min with a factor 4 for the
# handful of operations: pow2 and zero-centred cases 5e-14 .. 1e-12, offset
# 1000 / sigma 0.1 -> 4e-10, offset 1e6 / sigma 0.01 -> 4e-6
def _noise_limit(c):
    y = SC.yardstick(c)
    (_, mu, sg), (_, mua, sga) = SC.fits(c)
    top = max(np.abs(mu).max(), np.abs(mua).max()) / min(sg.min(), sga.min())
    if y is not None:
        (_, mu, sg), (_, mua, sga) = SC.fits(y)
        top = max(top, max(np.abs(mu).max(), np.abs(mua).max()) / min(sg.min(), sga.min()))
    lim = 4 * 50 * 2.0 ** -52 * max(top, 1.0)
    if c.kind.startswith("q"):
        # a quantized density is a sum of differences of cdf values, each good
        # to 2^-53 absolute: relative 2^-52 / p on the smallest cell mass p,
        # twice (below and above), in the case and in the yardstick
        _, ref = SC.oracle_scores(c)
        ll = np.concatenate([ref["below_llik"], ref["above_llik"]])
        lim += 4 * 2.0 ** -52 / np.exp(ll[np.isfinite(ll)].min())
    return lim


@pytest.mark.parametrize("c", [c for c in SC.CASES if c.group != "tiny"], ids=lambda c: c.name)
def test_scores_agree_with_the_yardstick(c):
    """The oracle's below - above scores of an image equal its yardstick's
    (candidate by candidate; the same argmax unless two candidates are within
    that disagreement), and oracle_noise records the largest difference."""
    noise = SC.oracle_noise(c)
    print("oracle_noise[%s] = %.3g (limit %.3g)" % (c.name, noise, _noise_limit(c)))
    assert noise <= _noise_limit(c)
    if c.group == "canon":
        return
    s, ref = SC.oracle_scores(c)
    y, yref = SC.oracle_scores(SC.yardstick(c))
    if ref["best"] != yref["best"]:
        assert abs(s[ref["best"]] - s[yref["best"]]) <= 2 * noise
    if c.group == "pow2":
        assert noise <= 1e-14 and ref["best"] == yref["best"]


@pytest.mark.parametrize("c", [c for c in SC.CASES if c.group == "tiny"], ids=lambda c: c.name)
def test_tiny_cases_reach_the_eps_floors(c):
    """A fitted bandwidth below EPS (so max(sigma, EPS) and
    max(sqrt2 sigma, EPS) are taken), and scores that are NOT the canonical
    ones: the reference is not scale-invariant here."""
    (_, _, sg), (_, _, sga) = SC.fits(c)
    assert min(sg.min(), sga.min()) < O.EPS
    assert np.sqrt(2.0) * sga.min() < O.EPS
    s, _ = SC.oracle_scores(c)
    y, _ = SC.oracle_scores(SC.case(c.canon))
    assert np.max(np.abs(s - y)) > 1e-3


@pytest.mark.parametrize("c", SC.CONT, ids=lambda c: c.name)
def test_oracle_sampler_passes_the_distribution_check(c):
    """KS_N draws of O.gmm1_sample / O.lgmm1_sample against
    O.truncated_mixture_cdf of the same posterior, p > KS_P: the check of
    tests/test_gpu_scales.py holds for the reference at every scale."""
    fam, _, _, _, low, high, _ = SC.spec(c)
    (w, mu, sg), _ = SC.fits(c)
    draw = O.gmm1_sample if fam == "GMM1" else O.lgmm1_sample
    x = draw(w, mu, sg, low=low, high=high, rng=np.random.RandomState(c.key % 2 ** 31),
             size=SC.KS_N)
    assert np.all(SC.in_support(c, x)) or fam == "LGMM1"
    y = np.log(x) if fam == "LGMM1" else x
    ks = stats.kstest(y, lambda v: O.truncated_mixture_cdf(v, w, mu, sg, low, high))
    print("oracle KS %s: D = %.5f p = %.3g" % (c.name, ks.statistic, ks.pvalue))
    assert ks.pvalue > SC.KS_P
