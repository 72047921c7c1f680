"""Every fit, count and scoring path at linear forgetting, prior weight and
gamma away from their defaults (25, 1.0, 0.25) -- tests/settings_cases.py.

The reference never passes linear_forgetting on from tpe.suggest, so the
chain of evidence is: the reference's unit functions -> the oracle
(tests/golden/units_settings.npz, tests/test_oracle_golden.py) -> the kernels
(here).  Tolerances are tests/test_gpu_posteriors.py's: means and bandwidths
bit for bit, Parzen weights rtol 1e-12 (the device sums the normaliser in
another order), categorical and randint probabilities bit for bit; scores at
the north_star tolerances of tests/test_gpu_parity.py.
tests/test_settings_cases.py shows, with the oracle alone, that the below
sets here carry ramps, that the winners lead by more than those tolerances,
and that three seeded slips (ramp endpoint not pinned, ramp indexed by history
row, (K*pw)*p) would be seen.  Made one at a time in the kernel source on a
scratch build, each fails here: the unpinned endpoint in the `pin` uploaded
counts, the history counts and the randint column of `fit lf=1 T=26`; the
row-indexed ramp in 17 of the 18 history fits and all three suggest tests; the
product order in the uploaded and history counts.
(Labels fitted in log space compare their means at 2 ulp: see _check_fit.)
"""
import functools

import numpy as np
import pytest

from oracle import tpe_oracle as O
from tests import settings_cases as SC
from tests.golden_io import load
from tests.test_gpu_sorted_fit import SPACE, _engines, _same_posteriors

pytestmark = pytest.mark.gpu

SET, SMETA = load("units_settings")
UNIT_LF = sorted({m["lf"] for m in SMETA["parzen"]})


@pytest.fixture(scope="module")
def engine():
    from hyperopt_amd.engine import Engine
    return Engine()


@pytest.fixture(scope="module")
def fit_engines():
    return _engines()  # (sorted_fit = True, sorted_fit = False)


def _check_fit(got, want, msg, log=False):
    """Means and bandwidths bit for bit, weights within rtol 1e-12.  ``log``:
    a label fitted in log space.  Its means are log(x) from the device's libm
    on one side and numpy's on the other, each good to an ulp and not always
    the same one (measured: 2 of 19 means of the lognormal column at T = 26
    differ by 1.1e-16), so no fit could make them equal: they take the
    tolerances tests/test_gpu_sorted_fit.py already gives such a column -- 2
    ulp (4.5e-16) for the means, and 1e-12 for the bandwidths, differences of
    two means of size <= 7 that are clipped to >= prior_sigma / 100 >= 0.01:
    4 * 2^-53 * 7 / 0.01 = 3e-13.  The two device fits still agree bit for
    bit on these columns (_same_posteriors)."""
    gw, gmu, gsig = got
    ow, omu, osig = want
    if log:
        np.testing.assert_allclose(gmu, omu, rtol=4.5e-16, atol=0, err_msg=msg)
        np.testing.assert_allclose(gsig, osig, rtol=1e-12, atol=0, err_msg=msg)
    else:
        np.testing.assert_array_equal(gmu, omu, err_msg=msg)
        np.testing.assert_array_equal(gsig, osig, err_msg=msg)
    np.testing.assert_allclose(gw, ow, rtol=1e-12, atol=0, err_msg=msg)


# ---------------------------------------------------------------------------
# the upload fit (tpe_parzen_fit)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pw", SMETA["prior_weights"])
@pytest.mark.parametrize("lf", UNIT_LF)
def test_upload_fit_on_the_reference_units(engine, lf, pw):
    """Every list of the fixture at this LF as one label of a level: the below
    half is the reference's own list (compared with the recorded arrays and
    with the oracle), the above half the same values in reverse tid order --
    another ramp over the same means."""
    from hyperopt_amd.engine import LabelWork
    ids = [i for i, m in enumerate(SMETA["parzen"]) if m["lf"] == lf]
    works = []
    for i in ids:
        m = SMETA["parzen"][i]
        obs = SET["parzen%d_obs" % i]
        works.append(LabelWork("x%d" % i, "normal", (m["prior_mu"], m["prior_sigma"]), obs,
                               obs[::-1].copy()))
    res = engine.run(works, prior_weight=pw, lf=lf, posteriors=True)
    for i, w, r in zip(ids, works, res):
        msg = "lf=%d n=%d pw=%g" % (lf, w.obs_below.size, pw)
        rec = tuple(SET["parzen%d_pw%g_%s" % (i, pw, k)] for k in ("w", "mu", "sigma"))
        _check_fit(r.extra["below"], rec, msg + " below (recorded)")
        for half, obs in (("below", w.obs_below), ("above", w.obs_above)):
            _check_fit(r.extra[half], O.adaptive_parzen_normal(obs, pw, 0.0, 10.0, lf),
                       "%s %s" % (msg, half))


@pytest.mark.parametrize("lf", [1, 2])
def test_upload_fit_ramp_end_at_the_sort_tile(engine, lf):
    """n = 2047, 2048, 2049: the ramp's last entry (position n - lf - 1) on
    either side of the 2048-observation sort tile, ties included."""
    from hyperopt_amd.engine import LabelWork
    rng = np.random.RandomState(77 + lf)
    obs = np.round(rng.normal(0, 2, 2049) * 8) / 8
    works = [LabelWork("x%d" % n, "normal", (0.0, 2.0), obs[:n], obs[:n][::-1].copy())
             for n in (2047, 2048, 2049)]
    for pw in (0.3, 7.5):
        res = engine.run(works, prior_weight=pw, lf=lf, posteriors=True)
        for w, r in zip(works, res):
            for half, o in (("below", w.obs_below), ("above", w.obs_above)):
                _check_fit(r.extra[half], O.adaptive_parzen_normal(o, pw, 0.0, 2.0, lf),
                           "n=%d %s pw=%g" % (o.size, half, pw))


# ---------------------------------------------------------------------------
# the fits from the resident history (tpe_fit_sorted; tpe_gather_obs + tpe_parzen_fit)
# ---------------------------------------------------------------------------
def _fit_works(name, n_cand=256):
    from hyperopt_amd.engine import LabelWork
    works = []
    for j, (lab, kind, a) in enumerate(SPACE):
        (below, _), (above, _) = SC.fit_lists(name, j)
        works.append(LabelWork(lab, kind, a, below, None, n_cand=n_cand, key=991 + j, col=j,
                               n_above=above.size))
    return works


def _check_fit_case(res, name, lf=None, tag=""):
    for j, (lab, kind, _) in enumerate(SPACE):
        want = SC.fit_expected(name, j, lf=lf)
        msg = "%s %s%s" % (name, lab, tag)
        if kind == "randint":
            np.testing.assert_array_equal(res[j].extra["p_below"], want[0], err_msg=msg)
            np.testing.assert_array_equal(res[j].extra["p_above"], want[1], err_msg=msg)
            continue
        log = kind in ("loguniform", "qloguniform", "lognormal")
        _check_fit(res[j].extra["below"], want[0], msg + " below", log)
        _check_fit(res[j].extra["above"], want[1], msg + " above", log)


def _histories(engines, mat, active, cap=32):
    from hyperopt_amd.engine import DeviceHistory
    out = []
    for eng in engines:
        h = DeviceHistory(eng, mat.shape[1], cap=cap)  # (grows while appending)
        h.append(mat, active)
        out.append(h)
    return out


@pytest.mark.parametrize("c", SC.group("fit"), ids=lambda c: c.name)
def test_history_fits(fit_engines, c):
    """Both fits of the resident history, 30 % of the rows inactive, up to 25
    below rows (a ramp on the BELOW side wherever the label keeps more than
    LF of them): the same bits from both, and the oracle's posterior of the
    lists gathered on the host in tid order."""
    mat, active, _, isb = SC.fit_history(c.name)
    srt, ref = fit_engines
    hs, hr = _histories(fit_engines, mat, active)
    works = _fit_works(c.name)
    kw = dict(prior_weight=c.pw, lf=c.lf, posteriors=True, is_below=isb)
    a = srt.run(works, history=hs, **kw)
    b = ref.run(works, history=hr, **kw)
    assert hs.order_rows and not hr.order_rows  # (the sorted fit ran on `srt` only)
    _same_posteriors(a, b)
    _check_fit_case(a, c.name)


def test_history_fit_through_a_permuted_row_list(fit_engines):
    """The history stored in another order than the trials' (rows= names each
    trial's row): the ramp follows the position in `rows`, not the stored row."""
    name = "fit lf=7 T=1025"
    c = SC.BY_NAME[name]
    mat, active, _, isb = SC.fit_history(name)
    perm = np.random.RandomState(1).permutation(mat.shape[0])
    stored, stored_act = np.empty_like(mat), np.empty_like(active)
    stored[perm], stored_act[perm] = mat, active
    works = _fit_works(name)
    out = []
    for eng, h in zip(fit_engines, _histories(fit_engines, stored, stored_act)):
        out.append(eng.run(works, prior_weight=c.pw, lf=c.lf, posteriors=True, history=h,
                           is_below=isb, rows=perm.astype(np.int32)))
    _same_posteriors(*out)
    _check_fit_case(out[0], name)


# ---------------------------------------------------------------------------
# categorical and randint counts: uploaded lists, the single-block history
# walk, the chunked walk
# ---------------------------------------------------------------------------
def _cat_specs():
    return [("c", "categorical", (SC.P_CAT,)), ("r", "randint", SC.RANDINT)]


def _check_counts(res, lists, pw, lf, msg):
    """lists: per label kind, ((below, rows), (above, rows)) as the label stores them."""
    (cb, _), (ca, _) = lists[0]
    (rb, _), (ra, _) = lists[1]
    np.testing.assert_array_equal(res[0].extra["p_below"],
                                  O.categorical_posterior(cb, pw, SC.P_CAT, lf), err_msg=msg)
    np.testing.assert_array_equal(res[0].extra["p_above"],
                                  O.categorical_posterior(ca, pw, SC.P_CAT, lf), err_msg=msg)
    np.testing.assert_array_equal(res[1].extra["p_below"],
                                  O.randint_posterior(rb, pw, *SC.RANDINT, lf=lf), err_msg=msg)
    np.testing.assert_array_equal(res[1].extra["p_above"],
                                  O.randint_posterior(ra, pw, *SC.RANDINT, lf=lf), err_msg=msg)


def _upload_count_works(below, above):
    from hyperopt_amd.engine import LabelWork
    low = SC.RANDINT[0]
    lists = [((below, None), (above, None)), ((below + low, None), (above + low, None))]
    works = [LabelWork(lab, kind, a, ls[0][0], ls[1][0])
             for (lab, kind, a), ls in zip(_cat_specs(), lists)]
    return works, lists


@pytest.mark.parametrize("c", SC.group("count_up"), ids=lambda c: c.name)
def test_counts_uploaded_lists(engine, c):
    """k_cat_counts: below lists with n - LF = 0, 1, 2, 3, above lists short
    and past one 1024-observation step; the `pin` lists, whose observation at
    the ramp's pinned last position is alone in its category."""
    works, lists = _upload_count_works(*SC.count_lists(c.name))
    res = engine.run(works, prior_weight=c.pw, lf=c.lf, posteriors=True)
    _check_counts(res, lists, c.pw, c.lf, c.name)


@functools.lru_cache(maxsize=None)
def _count_hist_works(T):
    from hyperopt_amd.engine import LabelWork
    lists = [SC.count_hist_lists(T, j) for j in (0, 1)]
    works = [LabelWork(lab, kind, a, ls[0][0].astype(float), None, col=j, n_above=ls[1][0].size)
             for j, ((lab, kind, a), ls) in enumerate(zip(_cat_specs(), lists))]
    return works, lists


@pytest.mark.parametrize("T", SC.COUNT_T)
def test_counts_in_the_history(engine, T):
    """k_cat_counts_hist (one window of 7 680 rows, and one row more) and the
    chunked k_cath_count / emit / fold (32 769 rows), at every (LF, prior
    weight) of the table on one resident history."""
    mat, active, isb = SC.count_history(T)
    hist, = _histories([engine], mat, active, cap=1024)
    works, lists = _count_hist_works(T)
    cases = [c for c in SC.group("count_hist") if c.n_below + c.n_above == T]
    assert len(cases) == 8
    for c in cases:
        res = engine.run(works, prior_weight=c.pw, lf=c.lf, posteriors=True, history=hist,
                         is_below=isb)
        _check_counts(res, lists, c.pw, c.lf, c.name)


# ---------------------------------------------------------------------------
# LF = 0 ("no forgetting", the reference's `if LF and ...`) and LF >= n
# ---------------------------------------------------------------------------
def test_no_forgetting_upload(engine):
    """Continuous labels at LF = 0, LF = n and LF > n equal the oracle at that
    LF (all weights 1); categorical labels at LF = 0 -- where the reference
    asserts -- give the bits of LF = n + 1."""
    from hyperopt_amd.engine import LabelWork
    rng = np.random.RandomState(5)
    obs = rng.normal(0, 2, 300)
    sizes = (0, 1, 2, 30, 300)
    works = [LabelWork("x%d" % n, "normal", (0.0, 2.0), obs[:n], obs[:n][::-1].copy())
             for n in sizes]
    cobs = rng.randint(0, len(SC.P_CAT), 1200)
    cworks, lists = _upload_count_works(cobs[:40], cobs)
    out = {}
    for lf in (0, 300, 1201):
        res = engine.run(works + cworks, prior_weight=0.3, lf=lf, posteriors=True)
        for w, r in zip(works, res):
            for half, o in (("below", w.obs_below), ("above", w.obs_above)):
                _check_fit(r.extra[half], O.adaptive_parzen_normal(o, 0.3, 0.0, 2.0, lf),
                           "lf=%d n=%d %s" % (lf, o.size, half))
        out[lf] = res[len(works):]
    _check_counts(out[1201], lists, 0.3, 1201, "lf = n + 1")
    _same_posteriors(out[0], out[1201])


def test_no_forgetting_history(fit_engines, engine):
    name = "fit lf=7 T=1025"
    c = SC.BY_NAME[name]
    mat, active, _, isb = SC.fit_history(name)
    works = _fit_works(name)
    for eng, h in zip(fit_engines, _histories(fit_engines, mat, active)):
        out = {}
        for lf in (0, 1025, 1026):
            out[lf] = eng.run(works, prior_weight=c.pw, lf=lf, posteriors=True, history=h,
                              is_below=isb)
            _check_fit_case(out[lf], name, lf=lf, tag=" lf=%d" % lf)
        _same_posteriors(out[0], out[1026])
    for T in (7681, 32769):  # the counts in the history, both walks
        mat, active, isb = SC.count_history(T)
        hist, = _histories([engine], mat, active, cap=1024)
        works, lists = _count_hist_works(T)
        out = [engine.run(works, prior_weight=1e-3, lf=lf, posteriors=True, history=hist,
                          is_below=isb) for lf in (0, T + 1)]
        _check_counts(out[1], lists, 1e-3, T + 1, "T=%d lf = n + 1" % T)
        _same_posteriors(*out)


# ---------------------------------------------------------------------------
# scores and winners
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.group("score"), ids=lambda c: c.name)
def test_scores_and_winners(engine, c):
    """2048 injected candidates per kind at (prior weight, LF) = (0.3, 7) and
    (7.5, 1), histories of 30 and 3000 points: both log-likelihood vectors
    and the winner, fp64 and fp32.  The winners' margins are asserted by
    tests/test_settings_cases.py."""
    from hyperopt_amd.engine import LabelWork
    below, above, cand = SC.score_inputs(c.name)
    ref = SC.score_expected(c.name)
    w = LabelWork(c.kind, c.kind, c.args, below, above, cand=cand)
    r64, = engine.run([w], prior_weight=c.pw, lf=c.lf, precision=64, outputs=True)
    np.testing.assert_allclose(r64.below_llik, ref["below_llik"], rtol=1e-6)
    np.testing.assert_allclose(r64.above_llik, ref["above_llik"], rtol=1e-6)
    assert r64.index == ref["best"]
    r32, = engine.run([w], prior_weight=c.pw, lf=c.lf, precision=32, outputs=True)
    np.testing.assert_allclose(r32.below_llik, ref["below_llik"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(r32.above_llik, ref["above_llik"], rtol=1e-4, atol=1e-4)
    assert r32.index == ref["best"]


# ---------------------------------------------------------------------------
# settings that change between calls on one engine
# ---------------------------------------------------------------------------
A, B = (1.0, 25), (0.3, 7)
T_CHG, NB_CHG = 3000, 25


@functools.lru_cache(maxsize=None)
def _change_inputs():
    from tests.test_gpu_replay import SPACE as RSPACE, _history
    mat, active, losses = _history(T_CHG, 31)
    active[:] = True  # (every label keeps all 25 below rows: a below ramp at LF = 7)
    # (no unbounded lattice: a WorkBatch key would have to name its range)
    space = [(j, e) for j, e in enumerate(RSPACE) if e[1] != "qnormal"]
    return mat, active, SC.split_rows(losses, NB_CHG), space


def _change_works(upload):
    from hyperopt_amd.engine import LabelWork
    mat, active, isb, space = _change_inputs()
    works = []
    for j, (lab, kind, a) in space:
        below, above = mat[isb == 1, j], mat[isb == 0, j]
        if upload:
            works.append(LabelWork(lab, kind, a, below, above, n_cand=1 << 16, key=4000 + j))
        else:
            works.append(LabelWork(lab, kind, a, below, None, n_cand=1 << 16, key=4000 + j, col=j,
                                   n_above=above.size))
    return works


def _bytes(res):
    if isinstance(res, list):
        cols = [[getattr(r, k) for r in res] for k in ("index", "value", "score", "n_scored")]
    else:
        cols = [getattr(res, k) for k in ("index", "value", "score", "n_scored")]
    return tuple(np.asarray(col, dt).tobytes()
                 for col, dt in zip(cols, (np.int64, np.float64, np.float64, np.int64)))


def _runner(mode):
    """An engine and a function (prior_weight, lf) -> result bytes of the one
    set of works in ``mode``."""
    from hyperopt_amd.engine import Engine, WorkBatch
    mat, active, isb, space = _change_inputs()
    eng = Engine()
    eng.native = mode not in ("upload", "history", "batch")
    if mode == "upload":
        works = _change_works(True)
        return eng, lambda pw, lf: _bytes(eng.run(works, prior_weight=pw, lf=lf))
    hist, = _histories([eng], mat, active, cap=4096)
    works = _change_works(False)
    if mode == "history":
        return eng, lambda pw, lf: _bytes(eng.run(works, prior_weight=pw, lf=lf, history=hist,
                                                  is_below=isb))

    def run(pw, lf):
        n = len(works)
        batch = WorkBatch(("settings-test",), [NB_CHG] * n, [T_CHG - NB_CHG] * n,
                          [w.key for w in works], [0] * n, lambda: works)
        return _bytes(eng.run(batch, prior_weight=pw, lf=lf, history=hist, is_below=isb))
    return eng, run


def _change_modes():
    from tests.test_gpu_replay import MODES
    return ["upload", "history", "batch"] + list(MODES)


@pytest.mark.parametrize("mode", _change_modes())
def test_settings_change_between_calls(mode):
    """One engine, one set of works, (prior weight, LF) = A, B, A with
    A = (1.0, 25), B = (0.3, 7): plans, batch plans and replay records are
    keyed by the settings, so the third result is the first's bytes, B's are a
    fresh engine's, and B is not A.  Each setting runs three times in a row
    -- a replaying engine records a level on its second call and re-issues it
    on the third -- and every call of a run gives the same bytes."""
    eng, run = _runner(mode)
    phases = []
    for pw, lf in (A, B, A):
        got = [run(pw, lf) for _ in range(3)]
        assert got[0] == got[1] == got[2], (mode, pw, lf)
        phases.append(got[0])
    assert phases[2] == phases[0]
    assert phases[1] != phases[0]
    _, fresh = _runner(mode)
    assert fresh(*B) == phases[1]
    if mode not in ("upload", "history", "batch"):
        st = eng.graph_stats
        assert st.get("replay", 0) + st.get("native", 0) >= 3, st


# ---------------------------------------------------------------------------
# end to end: tpe.suggest and suggest_many
# ---------------------------------------------------------------------------
def _mixed_space():
    from hyperopt_amd import hp
    from tests.golden import spaces
    return {"arch": spaces.nested(hp), "x": hp.uniform("x", -5, 5),
            "lr": hp.loguniform("lr", -7, 0), "q": hp.quniform("q", 0, 20, 1),
            "k": hp.randint("k", 3, 9),
            "c": hp.pchoice("c", [(0.1, 0), (0.2, 1), (0.3, 2), (0.15, 3), (0.25, 4)])}


@functools.lru_cache(maxsize=None)
def _study(T, seed):
    from hyperopt_amd import Trials, fmin, rand
    from hyperopt_amd.base import Domain
    space = _mixed_space()
    losses = iter(np.random.RandomState(seed).normal(size=T))
    trials = Trials()
    fmin(lambda p: float(next(losses)), space, algo=rand.suggest, max_evals=T, trials=trials,
         rstate=np.random.RandomState(seed), show_progressbar=False)
    return Domain(lambda p: 0.0, space), trials


def _vals(docs):
    return docs[0]["misc"]["vals"], docs[0]["misc"]["idxs"]


@pytest.mark.parametrize("n_ei", [24, 1 << 16])
def test_suggest_with_settings_device_history_matches_host_lists(monkeypatch, n_ei):
    """tpe.suggest through functools.partial(gamma=1.0, linear_forgetting=7,
    prior_weight=0.3) on about 700 trials of a mixed nested space
    (n_below = 25 > LF): the device-history path (WorkBatch levels, the sorted
    fit, counts in the history) and the host-list path (uploaded lists) give
    the same document (fp64 path at 24 candidates, fp32 table path at 2^16)."""
    from hyperopt_amd import tpe
    domain, trials = _study(700, 3)
    algo = functools.partial(tpe.suggest, gamma=1.0, linear_forgetting=7, prior_weight=0.3,
                             n_EI_candidates=n_ei, verbose=False)
    out = []
    for dev in (True, False):
        monkeypatch.setattr(tpe, "USE_DEVICE_HISTORY", dev)
        out.append([_vals(algo([700 + s], domain, trials, 11 + s)) for s in range(2)])
    assert out[0] == out[1]
    assert out[0][0] != out[0][1]  # (another seed, another document)
    monkeypatch.setattr(tpe, "USE_DEVICE_HISTORY", True)
    default = _vals(tpe.suggest([700], domain, trials, 11, gamma=1.0, n_EI_candidates=n_ei,
                                verbose=False))
    assert default != out[0][0]  # (the settings reach the kernels)


def test_suggest_many_over_two_settings():
    """Four studies holding two (prior weight, LF) pairs in one suggest_many
    (batched by those settings): each document equals the study's own
    tpe.suggest call."""
    from hyperopt_amd import tpe
    settings = [(0.3, 7), (7.5, 1), (0.3, 7), (7.5, 1)]
    reqs = []
    for s, ((pw, lf), T) in enumerate(zip(settings, (700, 700, 120, 260))):
        domain, trials = _study(T, 3 if T == 700 else 5 + s)
        reqs.append(tpe.SuggestRequest([T], domain, trials, 50 + s, gamma=1.0, prior_weight=pw,
                                       linear_forgetting=lf, n_EI_candidates=256))
    batched = tpe.suggest_many(reqs)
    singles = [tpe.suggest(rq.new_ids, rq.domain, rq.trials, rq.seed, verbose=False, **rq.kwargs)
               for rq in reqs]
    for s, (docs, single) in enumerate(zip(batched, singles)):
        assert _vals(docs) == _vals(single), s
    assert _vals(batched[0]) != _vals(batched[1])
