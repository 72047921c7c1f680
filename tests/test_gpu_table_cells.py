"""The cell table itself (tpe_table.hip: k_table_plan1/2, k_table_build,
k_table_score), cell by cell against the oracle, over all of |u| <= 1.0501.

The table's argmax is exact only if, on every cell and for every |u| <=
1.0501, (1) the stored polynomial is within eps_mix (relative) of its
mixture, (2) the score cubic is within its fit bound (<= kFitTol = 1e-6, the
job's maximum in eps_cubic) of off + ln P^_b - ln P^_a, and (3) a cell for
which either cannot be shown is flagged.  The other tests see these only at
drawn candidates, which never reach the tails or |u| > 1.  Here the table is
read back (tests/table_util.py) and every statement is evaluated in fp64 from
the stored numbers at fixed points of every cell (or of a fixed selection of
a large table's cells), with the oracle's log-densities as the reference:

  A  per mixture, unflagged cells: |m + ln P^(u) - L| <= eps_mix / (1 -
     eps_mix) + 2^-24 1.0001 |m| + delta; P^(u) > 0; P_0 in [1, 2]
  B  score, unflagged cells: |off + ln P^_b - ln P^_a - (L_b - L_a)| <=
     2.0001 eps_mix + 2^-24 1.0001 |off| + delta
  C  cubic, unflagged score cells: |q - (off + ln P^_b - ln P^_a)| <= 1e-6 (1
     + 1e-5); |q - (L_b - L_a)| <= eps_cubic + 2.0001 eps_mix + delta (what
     the band uses); |q'| <= slope; eps_cubic >= the cell's largest observed
     cubic error + 2^-21 sum_{k>=1} |c_k| 1.0501^k + 2^-24 |off| (the terms
     k_table_score adds to the fit bound)
  D  flags: a flagged cell has a flagged score cell; last_table_stats counts
     exactly the flagged cells / score cells below nb
  E  geometry: grid_of restated; [lo, hi] holds mu +- 5.8 sigma of every below
     component, clipped to the bounds; a 4096-candidate stream lies on the grid
  F  plan: reach_hi / reach_lo are the running max / reversed running min of
     plan_comp restated (relative 1e-12), the wide list and its counts, the
     admissible half-widths; eps_mix is mix_eps restated

delta = 1e-10 (1 + |L_b| + |L_a|) is the reference's own slack: fp64
log-sum-exp over <= 10^4 terms is good to ~1e-12 relative, and delta is more
than three orders below the smallest bound checked (4e-7).  Nothing here is
measured on the kernel.

The worst observed / bound ratios per assertion and kind are printed at the
end of the module, and each case prints the below-mixture mass of its flagged
score cells (capped: 1/50 for histories of 100 trials or more, 1/3 below).
"""
import numpy as np
import pytest

from oracle import tpe_oracle as O
from tests import band_util as B
from tests import table_util as TU
from tests.band_util import CONT

pytestmark = pytest.mark.gpu

N_CAND = 4096
U32 = 2.0 ** -24
U_FIXED = np.array(sorted(
    {0.0} | {s * v for s in (-1.0, 1.0) for v in (
        0.25, 0.5, 0.75, 1.0, 1.05 * np.cos(np.pi / 8), 1.05 * np.cos(3 * np.pi / 8), 1.05,
        1.0501)}))
ALL_CELLS = 2048   # tables of at most this many cells are checked whole
RATIO = {}         # (assertion, kind) -> worst observed / bound
_RUNS = {}         # case key -> Run (a case's table is built and checked once)


@pytest.fixture(scope="module")
def engine():
    from hyperopt_amd.engine import Engine
    yield Engine()
    _RUNS.clear()
    for a, kind in sorted(RATIO):
        print("table cells: %-3s %-10s worst observed / bound %.3g" % (a, kind, RATIO[(a, kind)]))


def _ratio(name, kind, err, bound):
    if err.size:
        r = float(np.max(err / bound))
        RATIO[(name, kind)] = max(RATIO.get((name, kind), 0.0), r)


# ---------------------------------------------------------------------------
# histories
# ---------------------------------------------------------------------------
def _frame(kind, args):
    """(a, b, to_x): a range of the kind's fitting coordinate that holds the
    prior's mass, and the map from it to an observation."""
    if kind in ("uniform", "loguniform"):
        a, b = args
    else:
        a, b = args[0] - 3.0 * args[1], args[0] + 3.0 * args[1]
    return float(a), float(b), (np.exp if kind in TU.LGMM else (lambda v: v))


def _draw(rng, kind, args, n):
    if kind in ("uniform", "loguniform"):
        v = rng.uniform(args[0], args[1], n)
    else:
        v = rng.normal(args[0], args[1], n)
    return np.exp(v) if kind in TU.LGMM else v


def _cluster(kind, args):
    """(300 + 6 observations: a cluster in 1 % of the range with 20 exact
    duplicates and three isolated points on each side; 25 with duplicates)."""
    a, b, to_x = _frame(kind, args)
    R, rng = b - a, np.random.RandomState(4100)
    c = a + R * (0.40 + 0.01 * rng.uniform(size=280))
    c = np.concatenate([c, np.repeat(c[17], 20)])
    iso = a + R * np.array([0.01, 0.05, 0.10, 0.80, 0.90, 0.99])
    big = rng.permutation(np.concatenate([c, iso]))
    s = a + R * rng.uniform(size=20)
    small = rng.permutation(np.concatenate([s, s[[3, 3, 3, 11, 11]]]))
    return to_x(big), to_x(small)


NEAR = [(0, 0), (1, 0), (1, 1), (2, 1)]
N_HIST = [3, 40, 2000]
N_TILE = [254, 255, 256, 511, 512]  # nc = n + 1 components: a plan tile, one over, two, one over


def _cases():
    """key -> (kind, args, below, above), every case of the module."""
    out = {}
    for kind, args in CONT:
        for nb_, na in NEAR:
            rng = np.random.RandomState(5100 + 10 * nb_ + na)
            out["near-prior-%s-%d-%d" % (kind, nb_, na)] = \
                (kind, args, _draw(rng, kind, args, nb_), _draw(rng, kind, args, na))
        for n in N_HIST:
            out["natural-%s-%d" % (kind, n)] = (kind, args) + tuple(
                np.asarray(v, np.float64) for v in B.history(kind, args, n, 7300 + n))
        for n in N_TILE:
            rng = np.random.RandomState(6100 + n)
            out["tiles-%s-%d" % (kind, n)] = \
                (kind, args, _draw(rng, kind, args, 25), _draw(rng, kind, args, n))
        big, small = _cluster(kind, args)
        out["cluster-%s" % kind] = (kind, args, small, big)
        if kind == "uniform":
            out["cluster-swapped-%s" % kind] = (kind, args, big, small)
    return out


CASES = _cases()


# ---------------------------------------------------------------------------
# one case: run, read back, check
# ---------------------------------------------------------------------------
class Run(object):
    pass


def _select(T):
    """The cells checked: all of a table of at most ALL_CELLS cells; of a
    larger one the first and last 128, 768 at a fixed stride, every cell that
    holds a component mean of either mixture and both neighbours of every
    flagged cell."""
    nb = T.nb
    if nb <= ALL_CELLS:
        return np.arange(nb)
    origin, h = float(T.tab["origin"]), float(T.tab["h"])
    mean = np.floor((np.concatenate([T.coef_b[:, 0], T.coef_a[:, 0]]) - origin) / (2.0 * h))
    mean = mean[(mean >= 0) & (mean < nb)].astype(np.int64)
    fl = np.flatnonzero(T.flagged | T.qflagged)
    nbr = np.concatenate([fl - 1, fl + 1])
    nbr = nbr[(nbr >= 0) & (nbr < nb)]
    stride = np.linspace(0, nb - 1, 768).astype(np.int64)
    return np.unique(np.concatenate([np.arange(128), np.arange(nb - 128, nb), stride, mean, nbr]))


def _check_cells(T, kind, args, below, above):
    """A, B, C and the per-cell part of D on the selected cells."""
    tab, sel = T.tab, _select(T)
    rng = np.random.RandomState(20260 + T.nb)
    U = np.concatenate([np.broadcast_to(U_FIXED, (sel.size, U_FIXED.size)),
                        rng.uniform(-TU.U_FIT, TU.U_FIT, (sel.size, 4))], axis=1)
    y, value = TU.cell_points(tab, sel, U, kind)
    Lb, La = TU.ref(kind, args, below, above, value)
    assert np.all(np.isfinite(Lb)) and np.all(np.isfinite(La))
    delta = 1e-10 * (1.0 + np.abs(Lb) + np.abs(La))
    eps_mix, eps_cubic = float(tab["eps_mix"]), float(tab["eps_cubic"])
    assert 0.0 < eps_mix < 5e-5 and 0.0 <= eps_cubic < 5e-6, tab
    ok, qok = ~T.flagged[sel], ~T.qflagged[sel]
    # D: a flagged cell has a flagged score cell (every cell below nb)
    assert not np.any(T.flagged & ~T.qflagged)
    Pb, Pa = TU.horner(T.Pb[sel], U), TU.horner(T.Pa[sel], U)
    # A: each mixture's stored polynomial against its mixture
    for name, P, P0, m, Lx in (("below", Pb, T.Pb[:, 0], T.m[sel, 0], Lb),
                               ("above", Pa, T.Pa[:, 0], T.m[sel, 1], La)):
        assert np.all(P[ok] > 0.0), name
        good = ~T.flagged
        assert np.all((P0[good] >= 1.0) & (P0[good] <= 2.0)), (name, P0[good].min(),
                                                               P0[good].max())
        with np.errstate(all="ignore"):
            err = np.abs(m[:, None] + np.log(P) - Lx)[ok]
        bound = (eps_mix / (1.0 - eps_mix) + U32 * 1.0001 * np.abs(m)[:, None] + delta)[ok]
        _ratio("A", kind, err, bound)
        bad = np.argwhere(~(err <= bound))
        assert bad.size == 0, ("A", name, kind, sel[ok][bad[0][0]], U[ok][tuple(bad[0])],
                               err[tuple(bad[0])], bound[tuple(bad[0])])
    # B: the score of the two stored polynomials
    off = T.off[sel][:, None]
    with np.errstate(all="ignore"):
        fhat = off + np.log(Pb) - np.log(Pa)
    err = np.abs(fhat - (Lb - La))[ok]
    bound = (2.0001 * eps_mix + U32 * 1.0001 * np.abs(off) + delta)[ok]
    _ratio("B", kind, err, bound)
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0, ("B", kind, sel[ok][bad[0][0]], U[ok][tuple(bad[0])],
                           err[tuple(bad[0])], bound[tuple(bad[0])])
    # C: the cubic
    q = T.q[sel]
    qu = TU.horner(q, U)
    e1 = np.abs(qu - fhat)[qok]
    _ratio("C1", kind, e1, np.full(e1.shape, 1e-6 * (1.0 + 1e-5)))
    bad = np.argwhere(~(e1 <= 1e-6 * (1.0 + 1e-5)))
    assert bad.size == 0, ("C fit", kind, sel[qok][bad[0][0]], U[qok][tuple(bad[0])],
                           e1[tuple(bad[0])])
    e2 = np.abs(qu - (Lb - La))[qok]
    b2 = (eps_cubic + 2.0001 * eps_mix + delta)[qok]
    _ratio("C2", kind, e2, b2)
    bad = np.argwhere(~(e2 <= b2))
    assert bad.size == 0, ("C band", kind, sel[qok][bad[0][0]], U[qok][tuple(bad[0])],
                           e2[tuple(bad[0])], b2[tuple(bad[0])])
    dq = np.abs(q[:, 1:2] + 2.0 * q[:, 2:3] * U + 3.0 * q[:, 3:4] * U * U)[qok]
    assert np.all(dq <= float(tab["slope"])), ("C slope", kind, dq.max(), float(tab["slope"]))
    if e1.size:
        ev = 2.0 ** -21 * (1.0501 * np.abs(q[:, 1]) + 1.1028 * np.abs(q[:, 2])
                           + 1.1581 * np.abs(q[:, 3])) + U32 * np.abs(T.off[sel])
        need = e1.max(axis=1) + ev[qok]
        _ratio("C3", kind, need, np.full(need.shape, eps_cubic))
        assert np.all(need <= eps_cubic), ("C eps_cubic", kind, need.max(), eps_cubic)
    return sel


def _check_geometry(eng, T, kind, args, below, above, work):
    """E, and what the stored bound says of the build's regime."""
    tab, job = T.tab, T.job
    origin, h, nb = TU.grid_of(tab, T.cap, T.coef_b.shape[0] + T.coef_a.shape[0])
    assert (float(tab["origin"]), float(tab["h"]), int(tab["nb"])) == (origin, h, nb)
    assert tab["inv_h"] == np.float32(1.0 / h) and tab["inv_w"] == np.float32(0.5 / h)
    lo, hi = float(tab["lo"]), float(tab["hi"])
    a, b = T.mu_b - TU.DRAW_Z * T.sigma_b, T.mu_b + TU.DRAW_Z * T.sigma_b
    low, high = O.posterior_spec(kind, args)[4:6]
    if low is not None:
        a, b = np.maximum(a, low), np.minimum(b, high)
        assert (job["low"], job["high"]) == (low, high)
    assert lo <= a.min() and b.max() <= hi, (lo, hi, a.min(), b.max())
    np.testing.assert_allclose([lo, hi], [a.min(), b.max()], rtol=1e-12, atol=0)  # and no wider
    s, = eng.run([work], precision=32, sample_only=True)
    with np.errstate(all="ignore"):
        ys = (np.log(s.cand) if kind in TU.LGMM else s.cand).astype(np.float32)
    assert ys.size == N_CAND and np.all(TU.band_cell(tab, ys) >= 0)


def _check_plan(T, reach=True):
    """F.  ``reach=False``: the level's band overflowed and the engine's exact
    re-score (tpe_score_pruned64) planned again into the same reach arrays,
    with its own exclusion margin -- the table's are gone; the wide list does
    not depend on the margin."""
    tab = T.tab
    TU.check_plan(T, reach=reach)
    # the stored bound is mix_eps of the build's deepest sum, cooperative or per wave
    coop = T.nb <= TU.COOP_CELLS
    want = TU.mix_eps(int(tab["build_items"]), coop)
    np.testing.assert_allclose(float(tab["eps_mix"]), want, rtol=1e-6)
    assert tab["build_ab"] == np.float32(TU.AB_MAX) and int(tab["build_items"]) >= 1


def _flag_mass(T, kind, args, below, above):
    """The below mixture's mass (of the sampler's accepted distribution) on
    the cells whose score cubic is flagged, from the oracle's exact CDF."""
    fl = np.flatnonzero(T.qflagged)
    if fl.size == 0:
        return 0.0
    fam, pmu, psig, tf, low, high, q = O.posterior_spec(kind, args)
    w, mu, sig = O.adaptive_parzen_normal(tf(np.asarray(below, np.float64)), 1.0, pmu, psig)
    origin, h = float(T.tab["origin"]), float(T.tab["h"])
    edges = origin + 2.0 * h * np.concatenate([fl, fl + 1]).astype(np.float64)
    cdf = O.truncated_mixture_cdf(edges, w, mu, sig, low, high)
    return float(np.sum(cdf[fl.size:] - cdf[:fl.size]))


def run_case(eng, case, cap=None, monkeypatch=None):
    """The case's table (CASES[case], under the cell budget ``cap``), built,
    read back and checked once (A-F)."""
    key = case if cap is None else "%s-cap-%d" % (case, cap)
    if key in _RUNS:
        return _RUNS[key]
    import hyperopt_amd.engine as E
    if cap is not None:
        monkeypatch.setattr(E, "TABLE_CAP", cap)
    kind, args, below, above = CASES[case]
    work = E.LabelWork(kind, kind, args, below, above, n_cand=N_CAND, key=0x7AB1E)
    R = Run()
    over = eng.band_overflows
    R.res, = eng.run([work], precision=32, scorer="table")
    R.overflowed = eng.band_overflows != over
    # (a band overflow makes the engine plan again, _check_plan; at the default
    # budget only the prior-only cases' flat score overflows, and theirs are
    # all wide components: F is checked whole)
    assert cap is not None or not R.overflowed or below.size + above.size == 0
    R.stats = dict(eng.last_table_stats)
    R.T = T = TU.read_table(eng, 0)
    R.kind, R.work = kind, work
    assert T.cap == (E.TABLE_CAP if cap is None else cap)
    # D: the level's counters are the flagged cells below nb, no others
    assert R.stats["failed_cells"] == int(T.flagged.sum()), R.stats
    assert R.stats["failed_score_cells"] == int(T.qflagged.sum()), R.stats
    R.sel = _check_cells(T, kind, args, below, above)
    _check_plan(T, reach=not R.overflowed)
    _check_geometry(eng, T, kind, args, below, above, work)
    R.mass = _flag_mass(T, kind, args, below, above)
    print("table cells: %-24s nb %6d  checked %5d  flagged %d / %d  below mass on flagged score "
          "cells %.3g" % (key, T.nb, R.sel.size, int(T.flagged.sum()), int(T.qflagged.sum()),
                          R.mass))
    _RUNS[key] = R
    return R


def _natural(eng, kind, n_hist):
    return run_case(eng, "natural-%s-%d" % (kind, n_hist))


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,args", CONT)
@pytest.mark.parametrize("sizes", NEAR)
def test_prior_only_and_near_it(engine, kind, args, sizes):
    R = run_case(engine, "near-prior-%s-%d-%d" % ((kind,) + sizes))
    assert (R.T.coef_b.shape[0], R.T.coef_a.shape[0]) == (sizes[0] + 1, sizes[1] + 1)


@pytest.mark.parametrize("kind,args", CONT)
@pytest.mark.parametrize("n_hist", N_HIST)
def test_natural_histories(engine, kind, args, n_hist):
    _natural(engine, kind, n_hist)


@pytest.mark.parametrize("kind,args", CONT)
@pytest.mark.parametrize("n_above", N_TILE)
def test_plan_tile_edges(engine, kind, args, n_above):
    R = run_case(engine, "tiles-%s-%d" % (kind, n_above))
    assert R.T.coef_a.shape[0] == n_above + 1


@pytest.mark.parametrize("kind,args", CONT)
def test_cluster_with_outliers(engine, kind, args):
    R = run_case(engine, "cluster-%s" % kind)
    T = R.T
    wide = T.wide_a[:int(T.tab["n_wide_above"])]
    assert T.coef_a.shape[0] == 307 and np.any(wide < 256) and np.any(wide >= 256), wide
    # some window component is on the wide list too (build_mix's skip)
    lo, hi = float(T.tab["lo"]), float(T.tab["hi"])
    assert np.any((T.coef_a[wide, 0] >= lo) & (T.coef_a[wide, 0] <= hi))


def test_cluster_with_outliers_roles_swapped(engine):
    R = run_case(engine, "cluster-swapped-uniform")
    wide = R.T.wide_b[:int(R.T.tab["n_wide_below"])]
    assert R.T.coef_b.shape[0] == 307 and np.any(wide < 256) and np.any(wide >= 256), wide


def test_both_build_regimes_are_covered(engine):
    """Among the natural histories one table builds cooperatively (a quad per
    block) and one per wave, and one is checked whole, one by selection."""
    small, large = _natural(engine, "uniform", 2000), _natural(engine, "normal", 2000)
    assert small.T.nb <= TU.COOP_CELLS and small.T.nb <= ALL_CELLS, small.T.nb
    assert large.T.nb > TU.COOP_CELLS + 1, large.T.nb
    assert large.sel.size < large.T.nb and large.sel.size >= 900


@pytest.mark.parametrize("cap", [1, 2, 3, 5, 4096, 4097])
def test_cap_limited_tables(engine, cap, monkeypatch):
    """The 2000-trial normal history under a cell budget below its natural
    cell count: nb is the cap, cells that cannot meet the bound are flagged,
    and A-D hold on every other one."""
    natural = _natural(engine, "normal", 2000)
    assert natural.T.nb > 4097, natural.T.nb
    R = run_case(engine, "natural-normal-2000", cap=cap, monkeypatch=monkeypatch)
    T = R.T
    assert T.nb == cap and T.cap == cap
    if cap <= 5:
        assert T.flagged.any()
    else:
        # 4096 builds cooperatively, 4097 per wave: _check_plan pins eps_mix to
        # mix_eps of the regime, and here the two regimes' values differ
        items = int(T.tab["build_items"])
        assert (T.nb <= TU.COOP_CELLS) == (cap == 4096)
        e_coop, e_wave = TU.mix_eps(items, True), TU.mix_eps(items, False)
        assert abs(e_coop - e_wave) > 1e-4 * e_coop
    if cap != 4096:
        assert T.nb % 4 != 0  # the last quad is partial


def test_three_jobs_in_one_launch(engine):
    """A job's cells, m pairs, score cells and table record do not depend on
    the jobs built beside it: the build has no floating-point atomics and its
    per-job grid does not depend on n_jobs."""
    import hyperopt_amd.engine as E
    cases = [CASES[k] + (run_case(engine, k),)
             for k in ("natural-uniform-2000", "natural-lognormal-40", "cluster-normal")]
    works = [E.LabelWork("%s%d" % (c[0], j), c[0], c[1], c[2], c[3], n_cand=N_CAND, key=0x7AB1E)
             for j, c in enumerate(cases)]
    engine.run(works, precision=32, scorer="table")
    stats = dict(engine.last_table_stats)
    tabs = [TU.read_table(engine, j) for j in range(3)]
    assert len({int(T.job["tbl_off"]) for T in tabs}) == 3
    for T, c in zip(tabs, cases):
        alone = c[4].T
        assert T.nb == alone.nb
        for got, want, what in zip(T.cell_bytes(), alone.cell_bytes(),
                                   ("cells", "m pairs", "score cells", "table record")):
            assert got == want, (c[0], what)
    assert stats["failed_cells"] == sum(int(T.flagged.sum()) for T in tabs)
    assert stats["failed_score_cells"] == sum(int(T.qflagged.sum()) for T in tabs)


@pytest.mark.parametrize("case", list(CASES))
def test_flagged_cells_hold_little_mass(engine, case):
    """What keeps the cases above from passing by testing nothing: at the
    default cell budget no cell is flagged, and the flagged score cells hold
    at most 1/50 of the below mixture's mass for a history of 100 trials or
    more, 1/3 below that (the mass of the sampler's accepted distribution on
    each flagged cell's interval, from the oracle's exact CDF).

    Measured on an MI355X: at most 0.001 on every uniform / loguniform case,
    at most 0.0093 on the normal / lognormal ones (tiles-512: 30 of 9033
    cells).  On the grid that the series bound alone admits, 14 uniform /
    loguniform cases missed the limit (natural-3: 0.44 / 0.35 against 1/3;
    25 below against 254..512 above components: 0.05 to 0.17 against 1/50;
    the cluster: 0.022); grid_of's refinement of small jobs answers that.
    """
    R = run_case(engine, case)
    n_trials = CASES[case][2].size + CASES[case][3].size
    assert R.stats["failed_cells"] == 0, R.stats
    assert R.mass <= (1.0 / 50 if n_trials >= 100 else 1.0 / 3), (R.mass, n_trials)
