"""The settings cases (tests/settings_cases.py) are sound, shown with the
oracle alone: the below sets tagged "below-ramp" do carry a ramp, the scoring
cases' winners lead by more than the tolerances tests/test_gpu_settings.py
compares with, and the table tells the oracle from each of three seeded slips
at exactly those tolerances -- so a kernel with one of them fails there.
"""
import numpy as np
import pytest

from oracle import tpe_oracle as O
from tests import settings_cases as SC
from tests.test_gpu_sorted_fit import SPACE


def test_case_table():
    assert len(SC.group("fit")) == 18 and len(SC.group("score")) == 40
    assert len(SC.group("count_up")) == 12 and len(SC.group("count_hist")) == 24
    for c in SC.CASES:
        assert isinstance(c.lf, int) and c.lf > 0 and (c.pw, c.lf) != (1.0, 25)
    assert {(c.lf, c.n_below + c.n_above) for c in SC.group("fit")} == \
        {(lf, T) for lf in (1, 7, 24) for T in (26, 1023, 1024, 1025, 2049, 5000)}
    for g in ("count_up", "count_hist"):
        assert {(c.lf, c.pw) for c in SC.group(g)} == \
            {(lf, pw) for lf in (1, 2, 7, 26) for pw in (0.3, 1e-3)}
    assert max(c.n_above for c in SC.group("count_up")) > 1024
    assert {c.n_below + c.n_above for c in SC.group("count_hist")} == {7680, 7681, 32769}
    assert {(c.pw, c.lf) for c in SC.group("score")} == {(0.3, 7), (7.5, 1)}
    assert {c.n_above for c in SC.group("score")} == {30, 3000}


def test_restatement_is_the_oracle():
    """parzen() / cat_post() / ramp_at() without a slip are the oracle, bit
    for bit -- the slips below differ from it by the slip alone."""
    for n in (0, 1, 2, 3, 8, 10, 15, 26, 27, 300):
        for lf in (1, 2, 7, 24, 26, 1000):
            want = O.linear_forgetting_weights(n, lf)
            np.testing.assert_array_equal(SC.ramp_at(np.arange(n), n, lf), want)
            rng = np.random.RandomState(n + lf)
            obs = rng.uniform(-5, 5, n)
            for pw in (1e-3, 0.3, 7.5):
                for a, b in zip(SC.parzen(obs, pw, 0.0, 10.0, lf),
                                O.adaptive_parzen_normal(obs, pw, 0.0, 10.0, lf)):
                    np.testing.assert_array_equal(a, b)
                cobs = rng.randint(0, 5, n)
                np.testing.assert_array_equal(SC.cat_post("categorical", cobs, pw, lf),
                                              O.categorical_posterior(cobs, pw, SC.P_CAT, lf))
                np.testing.assert_array_equal(
                    SC.cat_post("randint", cobs + 3, pw, lf),
                    O.randint_posterior(cobs + 3, pw, *SC.RANDINT, lf=lf))


def _below_sizes(c):
    if c.group == "fit":
        return [SC.fit_lists(c.name, j)[0][0].size for j in range(len(SPACE))]
    if c.group == "count_up":
        return [SC.count_lists(c.name)[0].size]
    if c.group == "count_hist":
        return [SC.count_hist_lists(c.n_below + c.n_above, j)[0][0].size for j in (0, 1)]
    return [SC.score_inputs(c.name)[0].size]


@pytest.mark.parametrize("c", [c for c in SC.CASES if "below-ramp" in c.tags],
                         ids=lambda c: c.name)
def test_below_sets_carry_a_ramp(c):
    """n_below > lf: LfRamp.ramp holds on the below side.  Every column of the
    case, except at LF = 24, where only the fully active column 0 keeps all 25
    below rows -- a ramp of one entry (num == 1)."""
    assert c.n_below > c.lf
    sizes = _below_sizes(c)
    if c.group == "fit" and c.lf == 24:
        assert sizes[0] == 25 and all(s <= 24 for s in sizes[1:])
    else:
        assert all(s > c.lf for s in sizes), sizes


def test_ramp_branches_are_all_reached():
    """n - lf of the below and above lists over the table: <= 0, 1, 2 and more."""
    seen = {0: set(), 1: set()}
    for c in SC.group("fit"):
        for j in range(len(SPACE)):
            for side, (obs, _) in enumerate(SC.fit_lists(c.name, j)):
                seen[side].add(min(max(obs.size - c.lf, 0), 3))
    for c in SC.group("count_up"):
        for side, obs in enumerate(SC.count_lists(c.name)):
            seen[side].add(min(max(obs.size - c.lf, 0), 3))
    assert seen[0] == {0, 1, 2, 3} and seen[1] >= {0, 3}, seen


@pytest.mark.parametrize("c", SC.group("score"), ids=lambda c: c.name)
def test_scoring_margins(c):
    """The oracle's best candidate leads the best candidate of any other value
    by more than the tolerance its scores are compared with: 1e-6 max(1, |s|)
    at fp64, 1e-4 max(1, |s|) at fp32 -- so `index == ref["best"]` is decided by
    the scores, not by rounding.  (A case that misses gets another seed in
    SCORE_SEEDS.)"""
    ref = SC.score_expected(c.name)
    assert np.all(np.isfinite(ref["below_llik"])) and np.all(np.isfinite(ref["above_llik"]))
    best, lead = SC.margin(c.name)
    print("%s: best %.6g lead %.3g" % (c.name, best, lead))
    assert lead > 1e-4 * max(1.0, abs(best))
    assert lead > 1e-6 * max(1.0, abs(best))


def _differs(a, b, rtol):
    if rtol == 0.0:
        return not np.array_equal(a, b)
    return bool(np.any(np.abs(a - b) > rtol * np.abs(b)))


def _slip_hits(slip):
    """Names of the cases (and which output) where the oracle restated with
    ``slip`` leaves the oracle at the GPU tests' tolerances: Parzen weights
    rtol 1e-12, categorical / randint probabilities bit for bit."""
    hits = []
    for c in SC.group("fit"):
        for j, (lab, kind, _) in enumerate(SPACE):
            good, bad = SC.fit_expected(c.name, j), SC.fit_expected(c.name, j, slip)
            for half, g, b in zip(("below", "above"), good, bad):
                if kind == "randint":
                    if _differs(b, g, 0.0):
                        hits.append((c.name, lab, half, "p"))
                elif _differs(b[0], g[0], 1e-12):
                    hits.append((c.name, lab, half, "w"))
    for c in SC.group("count_up") + SC.group("count_hist"):
        good, bad = SC.count_expected(c), SC.count_expected(c, slip)
        for kind in good:
            for half, g, b in zip(("below", "above"), good[kind], bad[kind]):
                if _differs(b, g, 0.0):
                    hits.append((c.name, kind, half, "p"))
    return hits


def test_slip_a_unpinned_endpoint_is_seen():
    """(a) the ramp's last entry computed as (num-1)*step + start instead of
    pinned to 1.0.  One ulp: invisible in Parzen weights at rtol 1e-12 (and no
    exposed output carries them more exactly), visible in the categorical /
    randint probabilities, which are compared bit for bit."""
    hits = _slip_hits("a")
    print("slip a:", len(hits), hits[:12])
    assert hits and all(h[3] == "p" for h in hits)
    for lf, n in SC.PINS:  # the premise of the pin cases
        assert SC.ramp_at(n - lf - 1, n, lf, pinned=False) != 1.0
    assert any(h[0].startswith("pin") for h in hits)


def test_slip_b_ramp_by_history_row_is_seen():
    """(b) the ramp indexed by the member's history row, not its rank among
    its set's active rows: below AND above sets of the history fits, and the
    history counts."""
    hits = _slip_hits("b")
    print("slip b:", len(hits))
    fit = {(h[0], h[2]) for h in hits if h[3] == "w"}
    for c in SC.group("fit"):
        if c.lf < 24:
            assert (c.name, "below") in fit, c.name
        if c.n_above * 0.5 > c.lf:
            assert (c.name, "above") in fit, c.name
    assert any(h[0].startswith("hist") for h in hits)
    assert not any(h[0].startswith(("up", "pin")) for h in hits)  # (uploaded lists have no rows)


def test_slip_c_pseudocount_product_order_is_seen():
    """(c) (K * pw) * p in place of K * (pw * p): the categorical kind only, at
    both prior weights."""
    hits = _slip_hits("c")
    print("slip c:", len(hits))
    assert hits and all(h[1] == "categorical" for h in hits)
    for pw in SC.COUNT_PW:
        assert any(SC.BY_NAME[h[0]].pw == pw for h in hits), pw
    for path in ("up", "hist T=7680", "hist T=7681", "hist T=32769"):
        assert any(h[0].startswith(path) for h in hits), path
