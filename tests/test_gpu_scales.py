"""Fits, samplers and scorers on search spaces far from unit scale
(tests/scale_cases.py; the cases are shown sound by tests/test_scale_cases.py
with the oracle alone): 2^-20 / 2^+20 images, offsets of 10^2 .. 10^6 spans,
log-space images, bandwidths below EPS, and bounds that fp32 rounds outward.

A power-of-two image must be the canonical result times 2^k BIT FOR BIT (fit,
fp64 stream, fp32 stream, winner index): every operation of the pipeline is
exact under a power-of-two scaling.  The other images are held to the oracle
at the suite's tolerances, and to the canonical case where a share or a path
is asserted.
"""
import numpy as np
import pytest
from scipy import stats

from oracle import streams as S
from oracle import tpe_oracle as O
from tests import scale_cases as SC
from tests import stream_cases as C

pytestmark = pytest.mark.gpu

N_STREAM = C.N_CAND          # fp64 stream: several blocks, a partial wave
N_TABLE = 1 << 16            # = TABLE_MIN_CAND: the table path
N_SMALL = 4096               # below it: pruned64 on the fp32 stream
N_OUTWARD = 1 << 20          # the outward cases' draws (a value on (float)low needs ~1e6 of them)


def _name(c):
    return c.name


def _skey(c):
    """A power-of-two image draws under its canonical case's key."""
    return SC.case(c.canon).key if c.group == "pow2" else c.key


def _work(c, **kw):
    from hyperopt_amd.engine import LabelWork
    return LabelWork(c.name, c.kind, c.args, c.below, c.above, key=_skey(c), **kw)


@pytest.fixture(scope="module")
def engine():
    from hyperopt_amd.engine import Engine
    return Engine()


@pytest.fixture(scope="module")
def dense64():
    from hyperopt_amd.engine import Engine
    e = Engine()
    e.exact64 = "dense"
    return e


def _scale(c):
    return 2.0 ** c.k if c.group == "pow2" else 1.0


# ---------------------------------------------------------------------------
# a. the fit
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def upload_fits(engine):
    res = engine.run([_work(c) for c in SC.CASES], posteriors=True)
    return {c.name: r.extra for c, r in zip(SC.CASES, res)}


@pytest.fixture(scope="module")
def history_fits():
    """The cases that are one history column each, fitted from a DeviceHistory
    with the order-merged fit (sorted_fit) and with the sort fit."""
    from hyperopt_amd.engine import DeviceHistory, Engine, LabelWork
    cases = [c for c in SC.CASES if c.obs is not None]
    mat = np.column_stack([c.obs for c in cases])
    out = {}
    for flag in (True, False):
        eng = Engine()
        eng.sorted_fit = flag
        h = DeviceHistory(eng, len(cases), cap=64)
        h.append(mat[:1000])
        h.append(mat[1000:])
        works = [LabelWork(c.name, c.kind, c.args, c.below, None, key=c.key, col=j,
                           n_above=c.above.size) for j, c in enumerate(cases)]
        res = eng.run(works, posteriors=True, history=h, is_below=SC.IS_BELOW)
        out[flag] = {c.name: r.extra for c, r in zip(cases, res)}
    return out


def _check_fit(c, got, what):
    """test_gpu_posteriors' rules: means and bandwidths to the last bit for the
    linear kinds (copies and differences of the observations); within rtol
    1e-12 for the log kinds (the device's log); weights within rtol 1e-12."""
    fam, _, _, _, low, high, _ = SC.spec(c)
    for half, ref in zip(("below", "above"), SC.fits(c)):
        w, mu, sg = got[half]
        if fam == "GMM1":
            np.testing.assert_array_equal(mu, ref[1], err_msg="%s %s mu" % (what, half))
            np.testing.assert_array_equal(sg, ref[2], err_msg="%s %s sigma" % (what, half))
        else:
            np.testing.assert_allclose(mu, ref[1], rtol=1e-12, atol=0)
            np.testing.assert_allclose(sg, ref[2], rtol=1e-12, atol=0)
        np.testing.assert_allclose(w, ref[0], rtol=1e-12, atol=0)
    if low is not None:
        for k, (w, mu, sg) in enumerate(SC.fits(c)):
            ref = np.sum(w * (O.normal_cdf(high, mu, sg) - O.normal_cdf(low, mu, sg)))
            np.testing.assert_allclose(got["p_accept"][k], ref, rtol=1e-12,
                                       err_msg="%s p_accept" % what)


@pytest.mark.parametrize("c", SC.CASES, ids=_name)
def test_fit(c, upload_fits, history_fits):
    _check_fit(c, upload_fits[c.name], "upload")
    if c.obs is not None:
        for flag in (True, False):
            _check_fit(c, history_fits[flag][c.name], "history sorted_fit=%s" % flag)
    if c.group == "pow2":
        s = _scale(c)
        paths = [(upload_fits[c.name], upload_fits[c.canon])] + [
            (history_fits[f][c.name], history_fits[f][c.canon]) for f in (True, False)]
        for got, canon in paths:
            for half in ("below", "above"):
                assert np.array_equal(got[half][0], canon[half][0])
                assert np.array_equal(got[half][1], canon[half][1] * s)
                assert np.array_equal(got[half][2], canon[half][2] * s)
            assert got["p_accept"] == canon["p_accept"]


# ---------------------------------------------------------------------------
# b. the fp64 scorers on injected candidates
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scored64():
    from hyperopt_amd.engine import Engine
    out = {}
    for mode in ("dense", "pruned"):
        eng = Engine()
        eng.exact64 = mode
        res = eng.run([_work(c, cand=c.cand) for c in SC.CASES], precision=64, outputs=True)
        out[mode] = {c.name: r for c, r in zip(SC.CASES, res)}
    return out


@pytest.mark.parametrize("c", SC.CASES, ids=_name)
def test_fp64_scorers(c, scored64):
    """Log-densities within rtol 1e-6 of the oracle (north_star), pruned
    within 1e-13 of dense (test_gpu_pruned64), and the oracle's argmax -- or a
    candidate the oracle scores within 4 oracle_noise of it (device and oracle
    each carry up to that rounding at the case's magnitude).  The tiny cases
    pin the EPS floors of the coefficients, the scorers and the cdfs."""
    s_ref, ref = SC.oracle_scores(c)
    d, p = scored64["dense"][c.name], scored64["pruned"][c.name]
    for r in (d, p):
        np.testing.assert_allclose(r.below_llik, ref["below_llik"], rtol=1e-6, atol=0)
        np.testing.assert_allclose(r.above_llik, ref["above_llik"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(p.below_llik, d.below_llik, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(p.above_llik, d.above_llik, rtol=1e-13, atol=1e-13)
    noise = SC.oracle_noise(c)
    for r in (d, p):
        print("%s: device index %d, oracle %d, oracle score gap %.3g (noise %.3g)"
              % (c.name, r.index, ref["best"], s_ref[ref["best"]] - s_ref[r.index], noise))
        if r.index != ref["best"]:
            assert s_ref[ref["best"]] - s_ref[r.index] <= 4 * noise
        assert r.value == c.cand[r.index]


# ---------------------------------------------------------------------------
# c. the fp64 stream
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream64(engine):
    res = engine.run([_work(c, n_cand=N_STREAM) for c in SC.CASES], precision=64,
                     sample_only=True)
    return {c.name: r.cand for c, r in zip(SC.CASES, res)}


def _stream_case(c, post):
    fam, _, _, _, low, high, q = SC.spec(c)
    w, mu, sg = post["below"]
    return C.Case(c.name, fam, w, mu, sg, low, high, _skey(c), N_STREAM, "scale"), \
        np.cumsum(w) / np.sum(w), mu, sg, q


@pytest.mark.parametrize("c", SC.CASES, ids=_name)
def test_fp64_stream(c, stream64, upload_fits):
    """Every candidate in [low, high) ([exp low, exp high) for the log kinds)
    and on the lattice; a power-of-two image is the canonical stream times
    2^k bit for bit; and every case is the Philox replay under
    test_gpu_streams' rules (1e-13 of the draw's terms; ambiguous candidates
    capped; quantized: the same lattice index except next to a half-integer)."""
    x = stream64[c.name]
    assert np.all(SC.in_support(c, x)), (x.min(), x.max())
    cc, cdf, mu, sg, q = _stream_case(c, upload_fits[c.name])
    if q is not None:
        assert np.all(SC.on_lattice(c, x))
    if c.group == "pow2":
        assert np.array_equal(x, stream64[c.canon] * _scale(c))
    rep = S.gmm_draw64(cdf, mu, sg, cc.key, np.arange(N_STREAM, dtype=np.int64), cc.low, cc.high)
    amb, tol = C.ambiguous64(cc, rep), C.tol64(rep, mu, sg)
    assert amb.sum() <= C.CAP64
    if q is None:
        y = np.log(x) if cc.family == "LGMM1" else x
        err = np.abs(y - rep["y"])
        # (the log of a stored value: its own rounding, 2^-52 max(1, |y|), on top)
        slack = 2.0 ** -52 * np.maximum(1.0, np.abs(y)) if cc.family == "LGMM1" else 0.0
        print("%s: max err / tol = %.3g" % (c.name, np.max(err[~amb] / tol[~amb])))
        assert np.all(err[~amb] <= tol[~amb] + slack)
    else:
        k_ref, half = C.quant_index(cc, rep, q, tol, fast_exp=False)
        assert half.sum() <= C.CAP_Q * N_STREAM
        ok = ~(amb | half)
        assert ok.sum() >= 0.98 * N_STREAM
        assert np.array_equal(np.rint(x / q)[ok].astype(np.int64), k_ref[ok])


# ---------------------------------------------------------------------------
# d. the fp32 suggest paths
# ---------------------------------------------------------------------------
def _exact_argmax(dense64, c, cand):
    """np.argmax over the dense fp64 scores of `cand` (test_gpu_table's)."""
    x, = dense64.run([_work(c, cand=cand)], precision=64, outputs=True)
    s64 = x.below_llik - x.above_llik
    best = int(np.argmax(s64))
    assert x.index == best
    return s64, best


def _job(engine):
    return engine.last_plan[3][0]


_suggested = {}


def _suggest(engine, dense64, c, n):
    """One label's precision-32 suggest at n candidates, its stream
    (sample_only), the exact argmax over that stream, and the path taken."""
    from hyperopt_amd import _lib as L
    if (c.name, n) not in _suggested:
        w = _work(c, n_cand=n)
        timers = {}
        r, = engine.run([w], precision=32, timers=timers)
        j = _job(engine)
        path = "table" if "table" in timers else \
            ("pruned64" if int(j["flags"]) & L.F_DRAW32 else "fp64")
        assert ("pruned64" in timers) == (path != "table"), sorted(timers)
        stats_ = engine.last_table_stats if path == "table" else None
        s, = engine.run([w], precision=32, sample_only=True)
        s64, best = _exact_argmax(dense64, c, s.cand)
        _suggested[(c.name, n)] = dict(r=r, cand=s.cand, s64=s64, best=best, path=path,
                                       stats=stats_)
    return _suggested[(c.name, n)]


@pytest.mark.parametrize("n", [N_TABLE, N_SMALL])
@pytest.mark.parametrize("c", SC.FP32, ids=_name)
def test_suggest_winner_is_the_exact_argmax(engine, dense64, c, n):
    """The table path (n = TABLE_MIN_CAND) and pruned64 on the fp32 stream
    (n = 4096): index, value and score are np.argmax of the dense fp64 scores
    of the stream sample_only materialises, first index on ties; every
    candidate lies in [low, high) of the fp64 bounds; the path is the case
    table's; a power-of-two image has the canonical fp32 stream times 2^k bit
    for bit and the same winner index.  uniform(1e6, 1e6+1) is the tie
    stress: fp32 holds 17 values of its support."""
    g = _suggest(engine, dense64, c, n)
    r, cand = g["r"], g["cand"]
    want = {"table": "table" if n >= N_TABLE else "pruned64", "fp64": "fp64"}[c.path]
    assert g["path"] == want, (g["path"], want)
    assert np.all(SC.in_support(c, cand)), (cand.min(), cand.max())
    print("%s n=%d: path %s, %d distinct values, stats %s"
          % (c.name, n, g["path"], np.unique(cand).size, g["stats"]))
    assert r.index == g["best"], (r.index, g["best"], g["s64"][r.index], g["s64"][g["best"]])
    assert r.value == cand[g["best"]] and r.n_scored == n
    np.testing.assert_allclose(r.score, g["s64"][g["best"]], rtol=1e-12, atol=1e-12)
    if g["stats"] is not None:
        assert g["stats"]["failed_cells"] == 0, g["stats"]
    if c.group == "pow2":
        g0 = _suggest(engine, dense64, SC.case(c.canon), n)
        assert np.array_equal(cand, g0["cand"] * _scale(c))
        assert r.index == g0["r"].index and g["path"] == g0["path"]


@pytest.mark.parametrize("c", [c for c in SC.FP32 if c.path == "table"], ids=_name)
def test_table_scores_within_the_reported_eps(engine, dense64, c):
    """table_scores at n = TABLE_MIN_CAND: every fp32 score within the eps the
    kernel reported for it, no slack; no failed cell; the share of candidates
    scored exactly equals the canonical case's on a power-of-two image and is
    at most n // 50 on uniform(1000, 1010) and normal(1e4, 0.5)
    (test_fast_table_scores_vs_oracle's limit for real histories)."""
    n = N_TABLE
    timers = {}
    fast, = engine.run([_work(c, n_cand=n)], precision=32, table_scores=True, timers=timers)
    assert "table" in timers
    st = dict(engine.last_table_stats)
    print("%s: %s" % (c.name, st))
    g = _suggest(engine, dense64, c, n)
    assert np.array_equal(fast.cand, g["cand"])
    score, eps = fast.extra["score"], fast.extra["eps"]
    err = np.abs(score - g["s64"])
    assert np.all(err <= eps), (np.max(err - eps), int(np.argmax(err - eps)))
    assert fast.index == g["best"]
    assert st["failed_cells"] == 0, st
    if c.group == "pow2":
        engine.run([_work(SC.case(c.canon), n_cand=n)], precision=32, table_scores=True)
        assert st["exact_candidates"] == engine.last_table_stats["exact_candidates"]
    if c.name in ("uniform(1000,1010)", "normal(1e4,0.5)"):
        assert st["exact_candidates"] <= n // 50, st


@pytest.mark.parametrize("c", [c for c in SC.FP32 if c.group == "outward"], ids=_name)
def test_outward_rounded_bounds_keep_the_support(engine, c):
    """2^20 draws with the below mass piled on `low`, whose fp32 image lies
    below it: none may leave [low, high) of the fp64 bounds."""
    s, = engine.run([_work(c, n_cand=N_OUTWARD)], precision=32, sample_only=True)
    x = s.cand
    inside = SC.in_support(c, x)
    assert inside.all(), (int((~inside).sum()), x.min() - (c.args[0] if c.kind == "uniform"
                                                            else np.exp(c.args[0])))


@pytest.mark.parametrize("side,mus", [("low", [-41.0, -40.0, -39.0]), ("high", [45.0, 46.0, 47.0])])
def test_clamped_fp32_draws_stay_inside_outward_rounded_bounds(side, mus):
    """A value ON the fp32 image of a bound, without waiting for one in 10^6
    draws: every attempt of a mixture 40 sigma outside (0.7, 1.3) is rejected
    and the draw is clamped -- to the smallest float >= 0.7, not to
    (float)0.7 = 0.69999999 < 0.7; on the other side to the largest float
    < 1.3.  The clamped values are the replay's, bit for bit."""
    from hyperopt_amd import _lib as L
    from hyperopt_amd.mixture import _Mixture
    from tests.test_gpu_streams import _sample
    c = C.Case("clamp-" + side, "GMM1", np.ones(3), np.array(mus), np.ones(3), 0.7, 1.3,
               0x0C1A3B00000000 + len(side), 257, "clamp")
    m = _Mixture(L.GMM1, c.w, c.mu, c.sigma, None, None)
    y = _sample(m, c, 32, 0)
    assert np.all((0.7 <= y) & (y < 1.3)), (y.min(), y.max())
    cdf, mu, sig = C.host_cdf(c)
    rep = S.gmm_draw32(cdf, mu, sig, c.key, C.indices(c, 0), c.low, c.high)
    assert rep["clamped"].all() and np.array_equal(y, rep["y"])
    want = np.nextafter(np.float32(0.7), np.float32(1)) if side == "low" else np.float32(1.3)
    assert np.all(y == float(want))  # ((float)1.3 < 1.3 is itself the largest float below 1.3)


@pytest.mark.parametrize("c", SC.FP32, ids=_name)
def test_stream_distribution(engine, c):
    """KS_N draws of the stream the precision-32 suggest scores (sample_only
    at precision 32) against the exact cdf of the oracle's truncated
    posterior, p > 1e-4 (test_gpu_sampler's threshold) -- what fp32 draws of
    uniform(1e6, 1e6+1), 17 values, cannot pass."""
    fam, _, _, _, low, high, _ = SC.spec(c)
    (w, mu, sg), _ = SC.fits(c)
    s, = engine.run([_work(c, n_cand=SC.KS_N)], precision=32, sample_only=True)
    y = np.log(s.cand) if fam == "LGMM1" else s.cand
    ks = stats.kstest(y, lambda v: O.truncated_mixture_cdf(v, w, mu, sg, low, high))
    print("KS %s: D = %.5f p = %.3g, %d distinct of %d"
          % (c.name, ks.statistic, ks.pvalue, np.unique(y).size, y.size))
    assert ks.pvalue > SC.KS_P


@pytest.mark.parametrize("cases", [SC.FP32, SC.QUANT], ids=["continuous", "quantized"])
def test_levels_equal_the_per_label_runs(engine, cases):
    """Each group's cases in ONE Engine.run with differing candidate counts
    (job offsets of a heterogeneous launch): exactly the per-label results."""
    ns = [(N_TABLE, N_SMALL, N_TABLE + 1021, 1000)[i % 4] for i in range(len(cases))]
    works = [_work(c, n_cand=n) for c, n in zip(cases, ns)]
    level = engine.run(works, precision=32)
    for c, w, r in zip(cases, works, level):
        one, = engine.run([w], precision=32)
        assert (r.index, r.value, r.score, r.n_scored) == \
            (one.index, one.value, one.score, one.n_scored), c.name
        assert np.all(SC.in_support(c, np.array([r.value]))), (c.name, r.value)
        if c.kind.startswith("q"):
            assert SC.on_lattice(c, r.value), (c.name, r.value)


def test_fmin_at_precision_32_resolves_a_narrow_far_space():
    """hp.uniform("t", 1e6, 1e6 + 1) beside an ordinary label through fmin
    and tpe.suggest at precision 32 (the level as a batch on the device
    history, its plan recorded and re-used as the history grows): the
    suggestions stay in [low, high), leave fp32's grid of 1/16 at 1e6, and
    lie closer to the optimum at 1e6 + 0.3 than draws from the prior."""
    from functools import partial

    from hyperopt_amd import Trials, fmin, hp, tpe
    trials = Trials()
    fmin(lambda p: (p["t"] - (1e6 + 0.3)) ** 2 + (p["x"] - 1.0) ** 2,
         {"t": hp.uniform("t", 1e6, 1e6 + 1), "x": hp.uniform("x", -5, 5)},
         algo=partial(tpe.suggest, precision=32, n_EI_candidates=4096, n_startup_jobs=10),
         max_evals=60, trials=trials, rstate=np.random.RandomState(3), show_progressbar=False)
    t = np.array([d["misc"]["vals"]["t"][0] for d in trials.trials])[10:]
    assert np.all((1e6 <= t) & (t < 1e6 + 1))
    off_grid = (t * 16.0) != np.rint(t * 16.0)
    assert off_grid.mean() > 0.9, off_grid.mean()
    # (draws from the prior have a median distance of 0.25 to the optimum)
    assert np.median(np.abs(t[-20:] - (1e6 + 0.3))) < 0.25


@pytest.mark.parametrize("c", SC.QUANT, ids=_name)
def test_quantized_path(engine, c):
    """The route of a drawn quantized label at precision 32 is the case
    table's: the lattice (or the dense fallback), drawing in fp32 only while
    the lattice indices stay within DRAW32_MAX_SLOT."""
    from hyperopt_amd import _lib as L
    timers = {}
    r, = engine.run([_work(c, n_cand=N_SMALL)], precision=32, timers=timers)
    j = _job(engine)
    path = "lat" if int(j["lat_n"]) > 0 else "qfb"
    assert path == c.path and path in timers, (path, sorted(timers))
    if c.draw32 is not None:
        assert bool(int(j["flags"]) & L.F_DRAW32) == c.draw32
    assert SC.on_lattice(c, r.value) and np.all(SC.in_support(c, np.array([r.value])))
