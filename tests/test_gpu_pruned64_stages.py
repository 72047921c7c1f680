"""The pruned exact fp64 scorer (csrc/tpe_pruned64.hip) stage by stage, on
the cases of tests/pruned_cases.py (whose premises tests/test_pruned_cases.py
proves on the CPU), with the dense fp64 kernel (tpe_score_continuous) beside
it wherever the statement applies to both:

  A  the plan at the exact margin, read back after the run (table_util.
     read_plan): [lo, hi] is min / max of mu -+ 8.7 sigma over the below
     components, clipped to the bounds and to the finite injected candidates
     (relative 1e-12); the floors are lc_prior - 0.5 far^2 - (log nc + 40)
     (relative 1e-12); reach windows, wide list and counts are statement F of
     test_gpu_table_cells.py (table_util.check_plan).  A second run with the
     same anchors and other candidates returns the same plan bit for bit.
  B  the pruning rule, candidate by candidate: with the window [first k with
     reach_hi[k] >= y, last k with reach_lo[k] <= y] plus the wide list, the
     omitted terms sum to at most e^-40 of the whole sum (longdouble) -- on
     the window edges themselves, the doubles next to them, the component
     means, lo and hi, each twice, one value 64 times and one 2048 times.
  C  below_llik / above_llik of both kernels against log sum_j exp(lc_j - 0.5
     ((y - mu_j) inv_j)^2) over every component in longdouble, from the
     read-back coefficients: rtol 1e-13, atol 1e-13 (test_gpu_pruned64.py's
     pruned-against-dense tolerance); the oracle at 1e-6; the winner is
     np.argmax of the kernel's own scores (first maximum) and within the
     tolerance of the reference's maximum.
  D  a value's two log-densities are the same bits wherever it stands: in
     another order, another tile, another candidate set, another batch.
  E  exp_neg64 on its own (tpe_exp_neg64_check) against mpmath / longdouble.

A candidate of an LGMM1 kind is injected as x = exp(y): the kernel scores
log(x), a double next to y, so there an edge is hit to within an ulp and by
its neighbours, and the references take log(x) in longdouble.

Tried once on scratch builds of the kernel: without the redo of an in-range
sum below 2^-900, test_threshold_path fails and test_gpu_pruned64.py does not
notice; `<` for `<=` in the window compare drops the window's last component
and fails nearly every test here (and test_gpu_pruned64.py's); `>` for `>=`
in first_ge changes no output bit anywhere -- the component it drops at y ==
reach_hi[k] is below the floor there, under 2^-53 of the sum, which is what B
states -- so no test can see it.

The worst observed / bound ratios of C per kind and kernel, the window share
of B and the worst exp_neg64 errors are printed at the end of the module.
"""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _lib as L
from oracle import tpe_oracle as O
from tests import pruned_cases as PC
from tests import table_util as TU

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-13    # test_gpu_pruned64.py: pruned against dense
RATIO = {}             # (kernel, kind) -> worst observed / bound of C
NOTES = []             # lines printed at the end of the module
_RUNS = {}


@pytest.fixture(scope="module")
def engine():
    from hyperopt_amd.engine import Engine
    assert np.finfo(np.longdouble).eps < 1e-18
    e = Engine()
    yield e
    e.exact64 = "auto"
    _RUNS.clear()
    for mode, kind in sorted(RATIO):
        print("pruned64 stages: C %-6s %-10s worst observed / bound %.3g"
              % (mode, kind, RATIO[(mode, kind)]))
    for line in NOTES:
        print("pruned64 stages: " + line)


def _work(c, cand, label=None):
    from hyperopt_amd.engine import LabelWork
    return LabelWork(label or c.kind, c.kind, c.args, c.below, c.above, cand=np.asarray(cand))


def _run(eng, mode, works):
    eng.exact64 = mode
    try:
        timers = {}
        res = eng.run(works, precision=64, outputs=True, timers=timers)
        assert ("pruned64" in timers) == (mode == "pruned")
    finally:
        eng.exact64 = "auto"
    return res


def _same_bits(a, b):
    """Equal as bits, NaNs as NaNs (whatever their payload)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = np.isnan(a)
    return np.array_equal(n, np.isnan(b)) and \
        np.array_equal(a[~n].view(np.uint64), b[~n].view(np.uint64))


def _plan_arrays(T):
    rec = [T.tab[n].tobytes() for n in ("lo", "hi", "h_below", "h_above", "n_wide_below",
                                        "n_wide_above", "T_below", "T_above")]
    return rec + [
        getattr(T, n + h).tobytes() for h in "ba" for n in ("coef_", "reach_hi_", "reach_lo_")
    ] + [T.wide_b[:int(T.tab["n_wide_below"])].tobytes(),
         T.wide_a[:int(T.tab["n_wide_above"])].tobytes(), T.mu_b.tobytes(), T.sigma_b.tobytes()]


def _halves(T):
    """[(coef, reach_hi, reach_lo, wide flags)] of the below / above mixture."""
    out = []
    for h, n in (("b", "n_wide_below"), ("a", "n_wide_above")):
        coef = getattr(T, "coef_" + h)
        wide = np.zeros(coef.shape[0], bool)
        wide[getattr(T, "wide_" + h)[:int(T.tab[n])]] = True
        out.append((coef, getattr(T, "reach_hi_" + h), getattr(T, "reach_lo_" + h), wide))
    return out


# ---------------------------------------------------------------------------
# A. the plan at the exact margin
# ---------------------------------------------------------------------------
def check_plan(c, T, cand):
    tab, job = T.tab, T.job
    assert job["flags"] & L.F_INJECTED and int(job["n_cand"]) == cand.size
    y = PC.to_y(c.kind, cand)
    y = y[np.isfinite(y)]
    assert (float(job["bin_lo"]), float(job["bin_hi"])) == (y.min(), y.max())
    for h in ("b", "a"):
        seg, coef = getattr(T, "seg_" + h), getattr(T, "coef_" + h)
        obs = c.below if h == "b" else c.above
        assert coef.shape[0] == obs.size + 1 == int(seg["n_obs"]) + 1
    np.testing.assert_array_equal(T.coef_b[:, 0], T.mu_b)
    np.testing.assert_allclose(T.coef_b[:, 1], 1.0 / T.sigma_b, rtol=1e-15, atol=0)
    lo, hi = float(tab["lo"]), float(tab["hi"])
    np.testing.assert_allclose([lo, hi], PC.plan_range(c.kind, c.args, T.mu_b, T.sigma_b, cand),
                               rtol=1e-12, atol=0)
    for coef, seg, name in ((T.coef_b, T.seg_b, "T_below"), (T.coef_a, T.seg_a, "T_above")):
        # (the fit places the prior on the device: found here by its mean and width)
        pos = np.flatnonzero((coef[:, 0] == float(seg["prior_mu"])) & (
            np.abs(coef[:, 1] * float(seg["prior_sigma"]) - 1.0) <= 1e-15))
        assert pos.size == 1, (c.name, name, pos)
        pos = int(pos[0])
        np.testing.assert_allclose(float(tab[name]), PC.floor_of(coef, pos, lo, hi), rtol=1e-12,
                                   atol=0)
    TU.check_plan(T)


# ---------------------------------------------------------------------------
# B. the pruning rule
# ---------------------------------------------------------------------------
def check_rule(c, T, cand):
    """-> the share of the components in each candidate's window, per half."""
    lo, hi = float(T.tab["lo"]), float(T.tab["hi"])
    y = PC.to_y(c.kind, cand)
    y = np.unique(y[(y >= lo) & (y <= hi)])
    assert y.size >= 10
    share = []
    for coef, rh, rl, wide in _halves(T):
        nc = coef.shape[0]
        k_lo = np.searchsorted(rh, y, side="left")        # first k with reach_hi[k] >= y
        k_hi = np.searchsorted(rl, y, side="right") - 1   # last k with reach_lo[k] <= y
        k = np.arange(nc)
        inc = ((k >= k_lo[:, None]) & (k <= k_hi[:, None])) | wide
        v = PC.terms(coef, y)
        e = np.exp(v - v.max(axis=1)[:, None])
        omitted, S = np.where(inc, 0, e).sum(axis=1), e.sum(axis=1)
        bad = np.flatnonzero(~(omitted <= np.exp(PC.LD(-TU.TAU_EXACT)) * S))
        assert bad.size == 0, (c.name, y[bad[:5]], omitted[bad[:5]] / S[bad[:5]])
        share.append(inc.sum(axis=1) / float(nc))
    return y, share


# ---------------------------------------------------------------------------
# C. values
# ---------------------------------------------------------------------------
def check_values(c, T, cand, res, mode, oracle=True, refs=None):
    refs = refs or [PC.reference(c.kind, coef, cand) for coef in (T.coef_b, T.coef_a)]
    for got, ref, side in ((res.below_llik, refs[0], "below"), (res.above_llik, refs[1], "above")):
        assert np.all(np.isfinite(ref))
        err = np.abs(got.astype(PC.LD) - ref).astype(np.float64)
        bound = ATOL + RTOL * np.abs(ref.astype(np.float64))
        r = float(np.max(err / bound))
        RATIO[(mode, c.kind)] = max(RATIO.get((mode, c.kind), 0.0), r)
        bad = np.flatnonzero(~(err <= bound))
        assert bad.size == 0, (c.name, mode, side, cand[bad[:5]], err[bad[:5]], bound[bad[:5]])
    np.testing.assert_array_equal(res.cand, cand)
    if oracle:
        with np.errstate(all="ignore"):
            o = O.continuous_label_scores(c.kind, c.args, c.below, c.above, cand)
        np.testing.assert_allclose(res.below_llik, o["below_llik"], rtol=1e-6)
        np.testing.assert_allclose(res.above_llik, o["above_llik"], rtol=1e-6)
    # the winner: argmax of the kernel's own scores, first maximum; and a
    # maximum of the reference's within twice the tolerance of its scores
    own = res.below_llik - res.above_llik
    assert res.index == O.broadcast_best_index(res.below_llik, res.above_llik), (c.name, mode)
    assert res.value == cand[res.index] and res.score == own[res.index]
    assert res.n_scored == cand.size
    sref = (refs[0] - refs[1]).astype(np.float64)
    slack = 2.0 * (2.0 * ATOL + RTOL * (np.abs(refs[0]) + np.abs(refs[1])).astype(np.float64))
    assert sref[res.index] >= sref.max() - slack[res.index] - slack[int(np.argmax(sref))]


def run_case(eng, name):
    """The case run twice with the pruned scorer (anchors + draws, then
    anchors + the first plan's edges + draws) and once with the dense kernel;
    A on both plans, B and C on the second set."""
    if name in _RUNS:
        return _RUNS[name]
    c = PC.case(name)
    first = PC.base_candidates(c)
    p1, = _run(eng, "pruned", [_work(c, first)])
    T1 = TU.read_plan(eng, 0)
    check_plan(c, T1, first)
    cand = PC.edge_candidates(c, _halves(T1), float(T1.tab["lo"]), float(T1.tab["hi"]))
    p, = _run(eng, "pruned", [_work(c, cand)])
    T = TU.read_plan(eng, 0)
    check_plan(c, T, cand)
    assert _plan_arrays(T) == _plan_arrays(T1), name   # candidate-independent, bit for bit
    d, = _run(eng, "dense", [_work(c, cand)])
    y, share = check_rule(c, T, cand)
    refs = [PC.reference(c.kind, coef, cand) for coef in (T.coef_b, T.coef_a)]
    check_values(c, T, cand, p, "pruned", refs=refs)
    check_values(c, T, cand, d, "dense", refs=refs)
    _RUNS[name] = (c, T, cand, p, d, y, share)
    return _RUNS[name]


@pytest.mark.parametrize("name", PC.STAGED)
def test_plan_rule_and_values(engine, name):
    c, T, cand, p, d, y, share = run_case(engine, name)
    # equal candidates, equal bits -- the run of 64, the tile of 2048, the pairs
    for res in (p, d):
        u, inv = np.unique(cand, return_inverse=True)
        for out in (res.below_llik, res.above_llik):
            first = np.zeros(u.size)
            first[inv[::-1]] = out[::-1]
            assert _same_bits(first[inv], out), name
    n = np.unique(cand, return_counts=True)[1]
    assert np.sum(n >= PC.RUN) >= 2 and n.max() >= PC.TILE and cand.size > PC.TILE + PC.RUN


def test_windows_prune(engine):
    """What keeps B from passing by including everything: on 2000 evenly
    spread above components of sigma = range / 100 the median candidate's
    window holds fewer than half of them (about a fifth: the reach is about
    ten sigma either way)."""
    c, T, cand, p, d, y, share = run_case(engine, "spread-uniform-2000")
    assert T.coef_a.shape[0] == 2001
    med = float(np.median(share[1]))
    NOTES.append("B window share, spread-uniform-2000 above: median %.3f, max %.3f (below: "
                 "median %.3f)" % (med, float(share[1].max()), float(np.median(share[0]))))
    assert 0.05 < med < 0.5, med


# ---------------------------------------------------------------------------
# C. candidates without a finite coordinate; the threshold path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,args", PC.CONT)
def test_non_finite_candidates(engine, kind, args):
    """+-inf, NaN and, for the LGMM1 kinds, 0, a negative value, the smallest
    subnormal and DBL_MAX among ordinary candidates: both kernels give NaN /
    +-inf in the same places and the same bits at those candidates (they are
    off the planned range: the pruned kernel's sum over every component is the
    dense kernel's), the same (index, value), and the ordinary candidates keep
    the tolerance of C."""
    c = PC.case("sizes-%s-25-255" % kind)
    base, sp = PC.base_candidates(c), PC.specials(kind)
    at = 2 + 11 * np.arange(sp.size)
    cand = np.insert(base, at, sp)
    at = at + np.arange(sp.size)
    assert _same_bits(cand[at], sp)
    p, = _run(engine, "pruned", [_work(c, cand)])
    T = TU.read_plan(engine, 0)
    check_plan(c, T, cand)
    d, = _run(engine, "dense", [_work(c, cand)])
    for a, b in ((p.below_llik, d.below_llik), (p.above_llik, d.above_llik)):
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert np.array_equal(np.isinf(a), np.isinf(b))
        assert np.array_equal(a[np.isinf(a)], b[np.isinf(b)])
        assert _same_bits(a[at], b[at]), (kind, cand[at], a[at], b[at])
        assert not np.all(np.isfinite(a[at]))
    assert (p.index, p.value) == (d.index, d.value) or (np.isnan(p.value) and np.isnan(d.value)
                                                        and p.index == d.index)
    ok = np.ones(cand.size, bool)
    ok[at] = False
    fin = cand[ok]
    for res, mode in ((p, "pruned"), (d, "dense")):
        for got, coef in ((res.below_llik, T.coef_b), (res.above_llik, T.coef_a)):
            ref = PC.reference(kind, coef, fin).astype(np.float64)
            np.testing.assert_allclose(got[ok], ref, rtol=RTOL, atol=ATOL)
        own = res.below_llik - res.above_llik
        if not np.any(np.isnan(own)):
            assert res.index == O.broadcast_best_index(res.below_llik, res.above_llik)


@pytest.mark.parametrize("kind,args", PC.THRESHOLD)
def test_threshold_path(engine, kind, args):
    """Candidates inside the planned range whose pruned sum is below 2^-900,
    subnormal or exactly 0 (test_pruned_cases.py: the sweep 33.0 ... 39.0
    between components at 0 and at 90) are redone over every component: both
    kernels keep the tolerance of C on the whole sweep."""
    c = PC.case("threshold-%s" % kind)
    cand = PC.base_candidates(c)
    p, = _run(engine, "pruned", [_work(c, cand)])
    T = TU.read_plan(engine, 0)
    check_plan(c, T, cand)
    d, = _run(engine, "dense", [_work(c, cand)])
    lo, hi = float(T.tab["lo"]), float(T.tab["hi"])
    y = PC.to_y(kind, cand[2:])
    assert np.all((y > lo) & (y < hi))
    for coef, rh, rl, wide in _halves(T):   # the device's fit keeps the CPU's premise
        s = PC.fast_sum(coef, y)
        assert np.sum(s >= PC.SLOW_BELOW) >= 5 and np.sum(s < PC.SLOW_BELOW) >= 5
        assert np.sum(s == 0.0) >= 1
        # no window component on the sweep: the fast sum is the wide list's
        if coef is T.coef_b:
            assert np.all(np.searchsorted(rh, y, side="left")
                          > np.searchsorted(rl, y, side="right") - 1)
    check_rule(c, T, cand)
    check_values(c, T, cand, p, "pruned")
    check_values(c, T, cand, d, "dense")
    assert np.all(np.isfinite(p.below_llik)) and np.all(np.isfinite(p.above_llik))


# ---------------------------------------------------------------------------
# D. bits do not depend on the neighbours
# ---------------------------------------------------------------------------
def _scored(eng, mode, c, values):
    """(below, above) of ``values`` scored behind the case's two anchors."""
    r, = _run(eng, mode, [_work(c, np.concatenate([PC.anchors(c), values]))])
    return r.below_llik[2:], r.above_llik[2:], r


@pytest.mark.parametrize("mode", ["pruned", "dense"])
def test_bits_do_not_depend_on_position(engine, mode):
    """4097 values as given, reversed, under a fixed permutation and split
    into candidate sets of 1, 63, 64, 65, 2047, 2048 and 2049: every value
    gets the same two doubles each time."""
    c, v = PC.case("neighbours"), PC.neighbour_list()
    bl, al, _ = _scored(engine, mode, c, v)
    perm = np.random.RandomState(9500).permutation(v.size)
    for order in (np.arange(v.size)[::-1], perm):
        b2, a2, _ = _scored(engine, mode, c, v[order])
        assert _same_bits(b2, bl[order]) and _same_bits(a2, al[order])
    off = 0
    for n in PC.SPLITS:
        idx = (off + np.arange(n)) % v.size
        off += n
        b2, a2, _ = _scored(engine, mode, c, v[idx])
        assert _same_bits(b2, bl[idx]) and _same_bits(a2, al[idx]), n
    assert off > v.size


@pytest.mark.parametrize("mode", ["pruned", "dense"])
def test_bits_do_not_depend_on_the_batch(engine, mode):
    """The 4097 values as one job of four, beside jobs of other kinds with 1,
    65 and 6000 candidates (the grid is sized by the largest job; the small
    jobs' spare blocks write empty records): the same bits, and every job
    returns the (index, value, score, n_scored) of its own run."""
    c, v = PC.case("neighbours"), PC.neighbour_list()
    works = [_work(c, np.concatenate([PC.anchors(c), v]), "j0")]
    for j, (kind, n) in enumerate((("loguniform", 1), ("normal", 65), ("lognormal", 6000))):
        cj = PC.case("sizes-%s-25-255" % kind)
        cand = PC.draws(cj, 1, seed=j) if n == 1 else \
            np.concatenate([PC.anchors(cj), PC.draws(cj, n - 2, seed=j)])
        works.append(_work(cj, cand, "j%d" % (j + 1)))
    assert [w.cand.size for w in works] == [4099, 1, 65, 6000]
    solo = [_run(engine, mode, [w])[0] for w in works]
    batch = _run(engine, mode, works)
    for s, b, w in zip(solo, batch, works):
        assert (s.index, s.value, s.score, s.n_scored) == (b.index, b.value, b.score, b.n_scored)
        assert b.n_scored == w.cand.size
        assert _same_bits(s.below_llik, b.below_llik) and _same_bits(s.above_llik, b.above_llik)


@pytest.mark.parametrize("kind,args", PC.CONT)
def test_bits_of_sampled_candidates(engine, kind, args):
    """test_pruned_equals_dense_sampled's shape at 4097 candidates: the
    drawn candidates injected again, shuffled, behind the anchors (the same
    planned range) get the same bits."""
    from hyperopt_amd.engine import LabelWork
    from tests.test_gpu_parity import _mixture_case
    rng = np.random.RandomState(len(kind))
    gen = _mixture_case(rng, kind, args, 1, 5000, 1)
    losses = rng.normal(size=5000)
    below, above = O.ap_split_trials(np.arange(5000), gen.obs_above, np.arange(5000), losses,
                                     0.25)
    c = PC.Case("sampled-%s" % kind, kind, args, below, above)
    w = LabelWork(kind, kind, args, below, above, n_cand=PC.N_NEIGHBOURS, key=77)
    for mode in ("pruned", "dense"):
        s, = _run(engine, mode, [w])
        assert s.cand.size == PC.N_NEIGHBOURS and s.n_scored == PC.N_NEIGHBOURS
        order = np.random.RandomState(9600).permutation(s.cand.size)
        bl, al, r = _scored(engine, mode, c, s.cand[order])
        assert _same_bits(bl, s.below_llik[order]) and _same_bits(al, s.above_llik[order]), mode
        if mode == "pruned":   # the anchors left the sampled job's range as it was
            T = TU.read_plan(engine, 0)
            lo, hi = PC.plan_range(kind, args, T.mu_b, T.sigma_b, PC.anchors(c))
            np.testing.assert_allclose([float(T.tab["lo"]), float(T.tab["hi"])], [lo, hi],
                                       rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------
# E. exp_neg64
# ---------------------------------------------------------------------------
EXP_REL = 3.25 * 2.0 ** -53   # table entry, the polynomial's last fma, the product: 2^-53
                              # each; 2^-57 truncation; the reduction
TINY = np.finfo(np.float64).tiny
DENORM = 2.0 ** -1074


def _exp_neg64(v):
    import torch
    lib = L.load()
    dv = torch.from_numpy(np.ascontiguousarray(v, np.float64)).cuda()
    out = torch.empty_like(dv)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.tpe_exp_neg64_check(dv.data_ptr(), dv.numel(), out.data_ptr(), st),
            "tpe_exp_neg64_check")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _exp_errors(v, got, ref):
    """(worst relative error of the normal results in units of 2^-53, worst
    error in ulps of the result, worst error of the subnormal results beyond
    the relative bound in units of 2^-1074, worst in those units), asserted."""
    ref64 = ref.astype(np.float64)
    err = np.abs(got.astype(PC.LD) - ref)
    normal = ref64 >= TINY
    rel = (err[normal] / ref[normal]).astype(np.float64)
    bad = np.flatnonzero(~(rel <= EXP_REL))
    assert bad.size == 0, (v[normal][bad[:5]], rel[bad[:5]] * 2.0 ** 53)
    ulps = (err[normal] / np.spacing(ref64[normal]).astype(PC.LD)).astype(np.float64)
    sub = ~normal
    over = (err[sub] - PC.LD(EXP_REL) * ref[sub]).astype(np.float64) / DENORM
    bad = np.flatnonzero(~(over <= 1.0))
    assert bad.size == 0, (v[sub][bad[:5]], over[bad[:5]])
    units = (err[sub].astype(np.float64) / DENORM)
    return (float(rel.max()) * 2.0 ** 53 if rel.size else 0.0, float(ulps.max()) if rel.size
            else 0.0, float(units.max()) if units.size else 0.0)


def test_exp_neg64():
    """exp_neg64 on 2^20 random arguments of [-746, 0], on every multiple of
    ln2 / 64 in range (the reduction's ties, where |r| is largest, and the
    multiples of ln2 / 32, where r is smallest) with both neighbours, around
    the -745.2 cut-off and at the special values.  Normal results: relative
    error <= 3.25 * 2^-53; subnormal results: the same plus 2^-1074; 1 at +-0;
    0 below -745.2, at -inf and at -1e300; NaN at NaN.

    Measured on an MI355X (1 255 218 arguments): normal results at most 2.724
    x 2^-53 relative, 1.923 ulp of the result; subnormal results at most
    1.000 unit of 2^-1074.  (A bit-exact CPU replay of the kernel's IEEE
    operations over 4e7 arguments gives 1.94 ulp and 1.38 units.)
    """
    import mpmath
    rng = np.random.RandomState(9700)
    ln2 = np.log(PC.LD(2))
    k = np.arange(0, int(746 * 64 / float(ln2)) + 1)
    ties = (-(k.astype(PC.LD)) * (ln2 / 64)).astype(np.float64)
    ties = ties[ties >= -746.0]
    bulk = np.concatenate([
        -746.0 * rng.uniform(size=1 << 20), ties, np.nextafter(ties, -np.inf),
        np.nextafter(ties, np.inf)])
    bulk = bulk[bulk <= 0.0]
    got = _exp_neg64(bulk)
    assert np.all(got[bulk < PC.EXP_CUT] == 0.0) and np.all(got >= 0.0) and np.all(got <= 1.0)
    live = bulk >= PC.EXP_CUT
    rel, ulps, units = _exp_errors(bulk[live], got[live], np.exp(bulk[live].astype(PC.LD)))
    # the special points against mpmath at 80 digits
    cut = -745.2
    pts = np.array([cut, np.nextafter(cut, 0.0), np.nextafter(cut, -np.inf), -745.13,
                    np.nextafter(-745.13, 0.0), np.nextafter(-745.13, -np.inf), -TINY,
                    -708.0, -708.4, -709.0, -1e-300, -1.0, -0.5 * float(ln2) / 32])
    g = _exp_neg64(pts)
    mpmath.mp.dps = 80
    for vi, gi in zip(pts, g):
        want = mpmath.exp(mpmath.mpf(float(vi)))
        if vi < cut:
            assert gi == 0.0
            continue
        err = abs(mpmath.mpf(float(gi)) - want)
        bound = mpmath.mpf(EXP_REL) * want + (mpmath.mpf(DENORM) if want < TINY else 0)
        assert err <= bound, (vi, gi, float(err / bound))
    sp = _exp_neg64(np.array([0.0, -0.0, -np.inf, -1e300, np.nan, np.nextafter(-745.2, -np.inf),
                              -746.0, -1e5]))
    assert sp[0] == 1.0 and sp[1] == 1.0 and np.all(sp[[2, 3, 5, 6, 7]] == 0.0) and np.isnan(sp[4])
    assert not np.signbit(sp[2]) and not np.signbit(sp[3])
    NOTES.append("E exp_neg64: normal results worst %.3f x 2^-53 relative (%.3f ulp of the "
                 "result), subnormal results worst %.3f x 2^-1074, %d arguments"
                 % (rel, ulps, units, bulk.size))
    print("pruned64 stages: " + NOTES[-1])
