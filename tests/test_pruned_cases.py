"""The pruned-scorer cases (tests/pruned_cases.py) are what they are named
for, shown with the oracle's fit alone: every case is within the size cap, the
anchors lie beyond mu +- 8.7 sigma of every below component (so the clip of the
planned range to the injected candidates is inactive, whatever else is
injected), the threshold sweep lies inside the restated range, straddles 2^-900
and reaches an exactly-zero fp64 sum while the oracle's log-densities stay
finite, and the longdouble reference is one.
tests/test_gpu_pruned64_stages.py runs the kernels on the same table.
"""
import numpy as np
import pytest

from oracle import tpe_oracle as O
from tests import pruned_cases as PC
from tests import table_util as TU


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).eps < 1e-18


def test_case_table():
    from tests.test_gpu_pruned64 import CONT
    assert PC.CONT == CONT and (TU.DRAW_Z64, TU.TAU_EXACT) == (8.7, 40.0)
    names = [c.name for c in PC.CASES]
    assert len(set(names)) == len(names)
    for kind, args in PC.CONT:
        for nb in (0, 3, 25):
            for na in (0, 1, 63, 64, 127, 255, 256, 512):
                c = PC.case("sizes-%s-%d-%d" % (kind, nb, na))
                assert (c.kind, c.args, c.below.size, c.above.size) == (kind, args, nb, na)
        c, s = PC.case("cluster-%s" % kind), PC.case("cluster-swapped-%s" % kind)
        assert (c.below.size, c.above.size) == (25, 306) == (s.above.size, s.below.size)
        assert np.unique(c.above).size < c.above.size      # exact duplicates
    c = PC.case("spread-uniform-2000")
    assert c.above.size == 2000 and np.unique(np.round(np.diff(np.sort(c.above)), 9)).size == 1
    w, mu, sigma = PC.fit(c, "above")
    assert np.all(np.delete(sigma, np.argmax(sigma)) == (c.args[1] - c.args[0]) / 100.0)
    c = PC.case("neighbours")
    assert (c.kind, c.below.size, c.above.size) == ("uniform", 25, 300)
    v = PC.neighbour_list()
    assert v.size == 4097 and 3800 < np.unique(v).size <= 3897
    assert PC.SPLITS == (1, 63, 64, 65, 2047, 2048, 2049) and sum(PC.SPLITS) > v.size
    assert PC.SWEEP.size == 61 and PC.SWEEP[0] == 33.0 and PC.SWEEP[-1] == 39.0
    assert np.allclose(np.diff(PC.SWEEP), 0.1, atol=1e-12)


@pytest.mark.parametrize("c", PC.CASES, ids=[c.name for c in PC.CASES])
def test_size_cap_and_anchors(c):
    """At most 2001 components x 4100 candidates; the anchors bracket mu +-
    8.7 sigma of every below component in the scoring coordinate, or sit at
    (or just beyond) the bounds: the restated range does not move when the
    anchors are the only candidates or when anything is added to them."""
    assert max(c.below.size, c.above.size) + 1 <= PC.MAX_COMP
    base = PC.base_candidates(c)
    # (7 values for each of at most 2 + 16 + 16 components of two mixtures, 6 at lo / hi, twice)
    assert base.size + 2 * (2 * 7 * 34 + 6) + PC.RUN + PC.TILE <= PC.MAX_CAND
    w, mu, sigma = PC.fit(c, "below")
    low, high = O.posterior_spec(c.kind, c.args)[4:6]
    a = PC.anchors(c)
    ya = PC.to_y(c.kind, a)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(ya)) and np.array_equal(base[:2], a)
    if low is None:
        assert ya[0] < np.min(mu - TU.DRAW_Z64 * sigma) and np.max(mu + TU.DRAW_Z64 * sigma) < ya[1]
    else:
        assert ya[0] <= low and high <= ya[1]
        assert PC.to_y(c.kind, np.nextafter(a[0], np.inf)) >= low
        assert PC.to_y(c.kind, np.nextafter(a[1], -np.inf)) <= high
    unclipped = (np.min(mu - TU.DRAW_Z64 * sigma), np.max(mu + TU.DRAW_Z64 * sigma))
    if low is not None:
        unclipped = (max(unclipped[0], low), min(unclipped[1], high))
    far = PC.to_x(c.kind, np.array([ya[0] - 50.0, ya[1] + 50.0]))
    for cand in (a, base, np.concatenate([base, far, PC.specials(c.kind)])):
        assert PC.plan_range(c.kind, c.args, mu, sigma, cand) == unclipped


@pytest.mark.parametrize("kind", [k for k, _ in PC.THRESHOLD])
def test_threshold_sweep(kind):
    """The sweep 33.0 ... 39.0 lies inside the restated range; the fp64 sum
    of both mixtures at the kernel's offset (the largest log-coefficient) has
    members at or above 2^-900 and below it, a subnormal one and an exact
    zero; the oracle's own log-densities are finite on all of it."""
    c = PC.case("threshold-%s" % kind)
    x = PC.base_candidates(c)
    assert x.size == 2 + 61
    w, mu, sigma = PC.fit(c, "below")
    assert mu.size == 26 and sigma[0] == 1.0 and sigma[1] == 1.0   # the prior at 0; 90: widest
    assert np.all(sigma[2:] < 0.25)
    lo, hi = PC.plan_range(c.kind, c.args, mu, sigma, x)
    y = PC.to_y(kind, x[2:])
    assert np.all((y > lo) & (y < hi)) and lo < -8.0 and hi > 98.0
    assert np.max(np.abs(y - PC.SWEEP)) <= 2 ** -47
    tiny = np.finfo(np.float64).tiny
    for side in ("below", "above"):
        s = PC.fast_sum(PC.oracle_coef(c, side), y)
        assert np.sum(s >= PC.SLOW_BELOW) >= 5 and np.sum(s < PC.SLOW_BELOW) >= 5, side
        assert np.any((s > 0.0) & (s < tiny)) or side == "above"
        assert np.sum(s == 0.0) >= 1, side
    with np.errstate(all="ignore"):
        ref = O.continuous_label_scores(c.kind, c.args, c.below, c.above, x)
    assert np.all(np.isfinite(ref["below_llik"])) and np.all(np.isfinite(ref["above_llik"]))
    # ... and equal the longdouble reference on the oracle's own coefficients
    for side in ("below", "above"):
        want = PC.reference(kind, PC.oracle_coef(c, side), x).astype(np.float64)
        np.testing.assert_allclose(ref[side + "_llik"], want, rtol=1e-9)


def test_reference_is_the_oracle():
    """The longdouble reference on the oracle's coefficients is the oracle's
    log-density (to the oracle's own fp64 error) for every kind: the -log x of
    the LGMM1 kinds and p_accept of the bounded GMM1 are in the right place."""
    for kind, args in PC.CONT:
        c = PC.case("sizes-%s-25-255" % kind)
        x = PC.base_candidates(c)
        with np.errstate(all="ignore"):
            ref = O.continuous_label_scores(c.kind, c.args, c.below, c.above, x)
        for side in ("below", "above"):
            want = PC.reference(kind, PC.oracle_coef(c, side), x).astype(np.float64)
            np.testing.assert_allclose(ref[side + "_llik"], want, rtol=1e-10, atol=1e-10)


def test_edge_values_from_a_restated_plan():
    """edge_values on a plan restated from the oracle's fit (plan_comp with
    the restated floor): both neighbours of every finite edge, every value
    twice, a run of 64 and a tile of 2048 equal values; within the cap."""
    c = PC.case("cluster-uniform")
    w, mu, sigma = PC.fit(c, "below")
    lo, hi = PC.plan_range(c.kind, c.args, mu, sigma, PC.base_candidates(c))
    plan = []
    for side in ("below", "above"):
        coef = PC.oracle_coef(c, side)
        psig = O.posterior_spec(c.kind, c.args)[2]
        pos = int(np.flatnonzero(coef[:, 1] == 1.0 / psig)[0])
        T = PC.floor_of(coef, pos, lo, hi)
        wide, hr, lr, hk = TU.plan_comp(coef, T, psig)
        rh = np.maximum.accumulate(hr)
        rl = np.minimum.accumulate(lr[::-1])[::-1]
        plan.append((coef, rh, rl, wide))
        assert wide[pos] and not wide.all()
    v = PC.edge_values(plan, lo, hi)
    u, n = np.unique(v, return_counts=True)
    assert np.all(n >= 2) and np.sum(n >= PC.RUN) >= 2 and n.max() >= PC.TILE
    for coef, rh, rl, wide in plan:
        k = PC.select(wide, coef.shape[0])
        assert {0, coef.shape[0] - 1} <= set(k.tolist())
        for e in np.concatenate([rh[k], rl[k]]):
            if np.isfinite(e):
                assert {np.nextafter(e, -np.inf), e, np.nextafter(e, np.inf)} <= set(u.tolist())
    assert PC.edge_candidates(c, plan, lo, hi).size <= PC.MAX_CAND
