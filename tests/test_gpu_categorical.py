"""The categorical path stage by stage -- the counts and k_cat_finalize
(csrc/tpe_fit.hip), k_score_cat<4|8|16>, k_score_cat_inj and k_cat_decide
(csrc/tpe_categorical.hip) -- on the cases of tests/cat_cases.py, whose
premises tests/test_cat_cases.py proves on the CPU: posterior bits in every K
regime of numpy's sum, launches that mix category counts, tied best scores,
categories of probability zero, and the prefix-first decision on rare ties.

All through Engine.run.  Every comparison is exact unless it states a
tolerance; the expected posteriors are the oracle's (the installed numpy's
np.sum), the expected streams and winners cat_cases' replay on the device's
own cumulative p.
"""
import numpy as np
import pytest

from oracle import tpe_oracle as O
from tests import cat_cases as CC

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def engine():
    from hyperopt_amd.engine import Engine
    return Engine()


def _works(jobs):
    from hyperopt_amd.engine import LabelWork
    return [LabelWork("c%d" % i, j.kind, j.args, j.below, j.above, n_cand=j.n_cand, key=j.key,
                      cand_base=j.cand_base, n_total=j.n_cand) for i, j in enumerate(jobs)]


def _device_cdfs(engine, n):
    """The below segments' cumulative p of the last level's n categorical
    works (all of its works), from the workspace."""
    csegs = engine.last_plan[1]
    assert len(csegs) == 2 * n
    end = int((csegs["p_off"] + csegs["n_cat"]).max())
    pool = engine._bufs["cat_cdf"][:8 * end].cpu().numpy().view(np.float64).copy()
    return [pool[int(c["p_off"]):int(c["p_off"]) + int(c["n_cat"])] for c in csegs[0::2]], \
        [pool[int(c["p_off"]):int(c["p_off"]) + int(c["n_cat"])] for c in csegs[1::2]]


def _rec(r):
    """A result as bytes and integers (NaN scores compare equal to themselves)."""
    return (np.float64(r.score).tobytes(), int(r.index), np.float64(r.value).tobytes(),
            int(r.n_scored))


def _run(engine, jobs, prefix, outputs=False, **kw):
    """(results, device cdfs of the below segments, need flags or None) of one
    level at engine.lat_prefix = prefix."""
    works = _works(jobs)
    old = engine.lat_prefix
    try:
        engine.lat_prefix = prefix
        rs = engine.run(works, precision=32, outputs=outputs, **kw)
    finally:
        engine.lat_prefix = old
    cdfs, _ = _device_cdfs(engine, len(jobs))
    need = None
    if prefix and not outputs and max(j.n_cand for j in jobs) > prefix:  # _score_cat's rule
        need = engine._bufs["cat_need"][:4 * len(jobs)].cpu().numpy().view(np.int32).copy()
    return rs, cdfs, need


# ---------------------------------------------------------------------------
# a. posterior bits by K regime
# ---------------------------------------------------------------------------
_worst = {"ratio": 0.0, "last": 0.0}


def _check_cdf(p, cdf, what):
    """The device's cumulative p of a posterior p (both from the device): it
    adds the same K numbers <= 1 as np.cumsum in another order, each add
    rounding by at most 2^-53, so the two differ by at most K 2^-52."""
    K = p.size
    assert np.all(np.diff(cdf) >= 0.0), what
    err = float(np.abs(cdf - np.cumsum(p)).max())
    ratio, last = err / (K * EPS), abs(float(cdf[-1]) - 1.0) / (K * EPS)
    _worst["ratio"], _worst["last"] = max(_worst["ratio"], ratio), max(_worst["last"], last)
    print("%s: max |cdf - cumsum| = %.3g = %.4f K 2^-52, |cdf[-1] - 1| = %.4f K 2^-52 (largest "
          "so far: %.4f, %.4f)" % (what, err, ratio, last, _worst["ratio"], _worst["last"]))
    assert err <= K * EPS and abs(float(cdf[-1]) - 1.0) <= K * EPS, what
    lo, hi = CC.intervals(cdf)
    wide = (p > 0.0) & (p * 4294967296.0 >= 2.0)
    assert np.all(hi[wide] > lo[wide]), what


@pytest.mark.parametrize("lf,pw", CC.SETTINGS)
@pytest.mark.parametrize("K", CC.POSTERIOR_K)
def test_posterior_bits_uploaded(engine, K, lf, pw):
    """tpe_cat_posterior on uploaded lists, randint(K) beside categorical with
    a Dirichlet prior: p_below and p_above are the oracle's bit for bit --
    through np_pw_leaf alone (K <= 128), the recursion, and past one
    8192-element numpy buffer -- and the cumulative p of each is monotone,
    within K 2^-52 of np.cumsum, with a word for every category of visible
    mass."""
    from hyperopt_amd.engine import LabelWork
    cases = [(kind,) + CC.posterior_case(K, kind) for kind in CC.KINDS]
    works = [LabelWork(kind, kind, args, below, above) for kind, args, below, above in cases]
    res = engine.run(works, posteriors=True, prior_weight=pw, lf=lf)
    cdf_b, cdf_a = _device_cdfs(engine, len(works))
    for i, (kind, args, below, above) in enumerate(cases):
        what = "K = %d %s lf=%d pw=%g" % (K, kind, lf, pw)
        for side, obs, cdf in (("below", below, cdf_b[i]), ("above", above, cdf_a[i])):
            got = res[i].extra["p_" + side]
            want = CC.posterior(kind, args, obs, pw, lf)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "%s %s: %d of %d entries differ, first %r != %r (numpy %s)" % (
                what, side, bad.size, K, got[bad[0]], want[bad[0]], np.__version__)
            np.testing.assert_array_equal(got, want)
            _check_cdf(got, cdf, what + " " + side)


@pytest.mark.parametrize("lf,pw", CC.SETTINGS)
@pytest.mark.parametrize("K", CC.HIST_K)
def test_posterior_bits_resident_history(engine, K, lf, pw):
    """tpe_cat_posterior_hist past 32 categories (k_cat_counts_hist, one block
    per category) on a DeviceHistory with inactive rows: the same bits."""
    from hyperopt_amd.engine import DeviceHistory, LabelWork
    mat, active, isb, p = CC.history_case(K)
    hist = DeviceHistory(engine, 2)
    hist.append(mat, active)
    specs = [("categorical", (tuple(p.tolist()),), 0), ("randint", (2, 2 + K), 2)]
    works, lists = [], []
    for j, (kind, args, off) in enumerate(specs):
        v = mat[active[:, j], j].astype(np.int64)
        b = isb[active[:, j]] == 1
        lists.append((v[b], v[~b]))
        works.append(LabelWork(kind, kind, args, v[b].astype(float), None, col=j,
                               n_above=int((~b).sum())))
    res = engine.run(works, posteriors=True, history=hist, is_below=isb, prior_weight=pw, lf=lf)
    cdf_b, cdf_a = _device_cdfs(engine, 2)
    for j, (kind, args, off) in enumerate(specs):
        for side, obs, cdf in (("below", lists[j][0], cdf_b[j]), ("above", lists[j][1], cdf_a[j])):
            if kind == "categorical":
                want = O.categorical_posterior(obs, pw, p, lf)
            else:
                want = O.randint_posterior(obs, pw, 2, 2 + K, lf=lf)
            got = res[j].extra["p_" + side]
            np.testing.assert_array_equal(got, want, err_msg="K = %d %s %s" % (K, kind, side))
            _check_cdf(got, cdf, "history K = %d %s lf=%d pw=%g %s" % (K, kind, lf, pw, side))


# ---------------------------------------------------------------------------
# b. mixed K in one launch
# ---------------------------------------------------------------------------
def _check_against_replay(jobs, rs, cdfs, need=None, streams=False):
    out = []
    for j, r, cdf in zip(jobs, rs, cdfs):
        rep = CC.replay(j, cdf)
        if streams:
            assert np.array_equal(r.cand.astype(np.int64), rep["k"]), j.name
            assert np.array_equal(r.cand, rep["k"].astype(np.float64)), j.name
        assert (r.index, r.value, r.n_scored) == (rep["index"], float(rep["value"]), j.n_cand), \
            (j.name, r.index, r.value, rep["index"], rep["value"])
        if need is not None:
            assert need[len(out)] == rep["need"], (j.name, need, rep["need"])
        out.append(rep)
    return out


def _mixed_level(engine, jobs):
    """The three runs of a level (per-candidate outputs; no outputs, every
    stream in full; prefix-first at 2^17 candidates): every job's record is
    its own single-job run's byte for byte, its stream the replay's on the
    device's cumulative p, its winner the replay's np.argmax."""
    long = [j._replace(n_cand=CC.N_PREFIXED) for j in jobs]
    for mode, js, prefix, outputs in (("outputs", jobs, CC.PREFIX, True),
                                      ("full", jobs, 0, False),
                                      ("prefix", long, CC.PREFIX, False)):
        rs, cdfs, need = _run(engine, js, prefix, outputs)
        assert (need is not None) == (mode == "prefix")
        _check_against_replay(js, rs, cdfs, need, streams=outputs)
        for i, j in enumerate(js):
            solo, scdf, sneed = _run(engine, [j], prefix, outputs)
            assert _rec(solo[0]) == _rec(rs[i]), (mode, j.name, solo[0], rs[i])
            assert np.array_equal(scdf[0], cdfs[i]), (mode, j.name)
            if need is not None:
                assert sneed[0] == need[i], (mode, j.name)
            if outputs:
                for a, b in ((solo[0].cand, rs[i].cand), (solo[0].below_llik, rs[i].below_llik),
                             (solo[0].above_llik, rs[i].above_llik)):
                    assert a.tobytes() == b.tobytes(), (mode, j.name)
                s = rs[i].below_llik - rs[i].above_llik
                assert rs[i].index == j.cand_base + int(np.argmax(s))
                assert np.float64(rs[i].score).tobytes() == s[np.argmax(s)].tobytes()


@pytest.mark.parametrize("name", sorted(CC.LEVELS))
def test_mixed_k_in_one_launch(engine, name):
    """launch_cat picks k_score_cat<KR> from the launch's largest K: a small K
    beside a large one runs under another instantiation (and a K <= 16 beside
    K = 300 next to the binary search and the plain argmax) with the same
    result as alone; n_cand 1001 beside 16 tiles and 3, cand_base 0 beside 3."""
    _mixed_level(engine, list(CC.level(name)))


# ---------------------------------------------------------------------------
# c. tied best categories
# ---------------------------------------------------------------------------
def _check_tie(jobs, rs, cdfs, need):
    later = 0
    for i, (j, r, cdf) in enumerate(zip(jobs, rs, cdfs)):
        if j.name.startswith("tie"):
            k = CC.draw(cdf, j.key, j.cand_base, j.n_cand)
            first = [int(np.flatnonzero(k == c)[0]) for c in CC.TIE_CATS]
            win = min(first)
            assert (r.index, int(r.value)) == (j.cand_base + win, int(k[win])), (j.name, r, first)
            assert int(r.value) in CC.TIE_CATS and r.n_scored == j.n_cand
            later += int(first[1] < first[0])
            if need is not None:
                assert max(first) < CC.PREFIX
                assert need[i] == 0 == CC.need_flag(k[:CC.PREFIX], CC.job_scores(j), cdf, j.n_cand)
    return later


@pytest.mark.parametrize("prefix", [0, CC.PREFIX])
@pytest.mark.parametrize("n_cand", CC.TIE_N)
def test_tied_best_categories(engine, n_cand, prefix):
    """Categories 0 and 5 score the same bits, the maximum: under every key the
    winner is the first candidate holding either (equal scores share a rank in
    k_score_cat's key), and the prefix-first decision needs no more than the
    prefix, which holds both."""
    jobs = list(CC.tie_jobs(n_cand))
    rs, cdfs, need = _run(engine, jobs, prefix)
    assert (need is not None) == (prefix > 0 and n_cand > prefix)
    later = _check_tie(jobs, rs, cdfs, need)
    assert later >= 2 and len(jobs) - later >= 2      # the larger category first, and the smaller
    _check_against_replay(jobs, rs, cdfs, need)
    assert len({_rec(r)[0] for r in rs}) == 1          # one score, whichever category won


@pytest.mark.parametrize("name", ["kr8", "all"])
def test_tied_best_categories_in_a_mixed_launch(engine, name):
    """The tie jobs between the jobs of a mixed level: under k_score_cat<8>
    (K = 8 in registers) and under <16> beside K = 300."""
    for n in CC.TIE_N:
        tie = [t._replace(n_cand=n, cand_base=b) for t, b in zip(CC.tie_jobs(n)[:4], (0, 3, 0, 3))]
        lvl = [j._replace(n_cand=n) for j in CC.level(name)] if n > CC.PREFIX else \
            list(CC.level(name))
        jobs = [x for pair in zip(lvl, tie) for x in pair] + lvl[len(tie):]
        for prefix in (0, CC.PREFIX):
            rs, cdfs, need = _run(engine, jobs, prefix)
            _check_tie(jobs, rs, cdfs, need)
            _check_against_replay(jobs, rs, cdfs, need)


# ---------------------------------------------------------------------------
# d. zero-probability categories
# ---------------------------------------------------------------------------
def _check_llik(r, k, job):
    """Per-candidate log-densities against the oracle's on the ids k: the
    -inf entries exactly, the finite ones at the project's rtol."""
    with np.errstate(all="ignore"):
        ref = O.categorical_label_scores(job.kind, job.args, job.below, job.above, k)
    for got, want in ((r.below_llik, ref["below_llik"]), (r.above_llik, ref["above_llik"])):
        inf = np.isneginf(want)
        assert np.array_equal(np.isneginf(got), inf) and np.all(np.isfinite(want[~inf]))
        np.testing.assert_allclose(got[~inf], want[~inf], rtol=1e-14, atol=0)
    return ref


def test_zero_probability_sampled(engine):
    """No candidate holds the NaN or the -inf category; the winner is the
    first candidate of the +inf category, with score +inf; the prefix-first
    decision is not reopened by the NaN category, which no word draws."""
    jobs = [CC.zero_job(key, n, base) for key, (n, base) in
            zip(CC.ZERO_KEYS, ((1001, 0), (CC.TILE * 16 + 3, 3), (1001, 3), (CC.TILE * 16 + 3, 0)))]
    rs, cdfs, _ = _run(engine, jobs, CC.PREFIX, outputs=True)
    for j, r, rep in zip(jobs, rs, _check_against_replay(jobs, rs, cdfs, streams=True)):
        k = rep["k"]
        assert not np.isin(r.cand, (CC.ZERO_NAN, CC.ZERO_NINF)).any()
        first = int(np.flatnonzero(k == CC.ZERO_PINF)[0])
        assert (r.index, r.value, r.score) == (j.cand_base + first, float(CC.ZERO_PINF), np.inf)
        _check_llik(r, k, j)
        assert np.all(np.isneginf(r.above_llik[k == CC.ZERO_PINF]))
    long = [j._replace(n_cand=1 << 17) for j in jobs]
    for prefix in (CC.PREFIX, 0):
        rs, cdfs, need = _run(engine, long, prefix)
        reps = _check_against_replay(long, rs, cdfs, need)
        for j, r, rep in zip(long, rs, reps):
            assert (r.value, r.score) == (float(CC.ZERO_PINF), np.inf) and r.index < CC.PREFIX + 3
            assert not np.isin(rep["k"], (CC.ZERO_NAN, CC.ZERO_NINF)).any()
            lo, hi = CC.intervals(cdfs[0])
            assert lo[CC.ZERO_NAN] == hi[CC.ZERO_NAN]      # on the device's cumulative p
        if prefix:
            assert need is not None and not need.any()


def test_zero_probability_last_category(engine):
    """The last category scoring NaN (observed on neither side, prior 0): it
    would beat every winner, but takes no word -- the word 2^32 - 1, below no
    saturated threshold, belongs to the last category with mass -- so the
    prefix-first decision stays closed and the records are the full stream's."""
    jobs = [CC.zero_job(key, 1 << 17, base, last_nan=True)
            for key, base in zip(CC.ZERO_KEYS, (0, 3, 0, 3))]
    score = CC.job_scores(jobs[0])
    assert np.isnan(score[[CC.ZERO_NAN, 5]]).all()
    pre, cdfs, need = _run(engine, jobs, CC.PREFIX)
    full, _, _ = _run(engine, jobs, 0)
    assert [_rec(r) for r in pre] == [_rec(r) for r in full]
    for cdf in cdfs:
        lo, hi = CC.intervals(cdf)
        assert lo[5] == hi[5] and lo[CC.ZERO_NAN] == hi[CC.ZERO_NAN] and int(hi[4]) == 1 << 32
    reps = _check_against_replay(jobs, pre, cdfs, need)
    assert need is not None and not need.any()
    for r, rep in zip(pre, reps):
        assert (r.value, r.score) == (float(CC.ZERO_PINF), np.inf)
        assert not np.isin(rep["k"], (CC.ZERO_NAN, 5)).any()


@pytest.mark.parametrize("with_nan,index", [(True, 6), (False, 3)])
def test_zero_probability_injected(engine, with_nan, index):
    """k_score_cat_inj on the ids (0, 2, 4, 3, 5, 3, 1, 0, 1): the first NaN
    wins, as in np.argmax; without the id 1 the first +inf."""
    from hyperopt_amd.engine import LabelWork
    j = CC.zero_job()
    ids = np.array([i for i in CC.ZERO_INJ if with_nan or i != CC.ZERO_NAN])
    w = LabelWork("z", j.kind, j.args, j.below, j.above, cand=ids.astype(float))
    for precision in (32, 64):
        r, = engine.run([w], precision=precision, outputs=True)
        ref = _check_llik(r, ids, j)
        assert ref["best"] == index
        assert (r.index, r.value) == (index, float(ids[index]))
        assert np.isnan(r.score) if with_nan else r.score == np.inf
        with np.errstate(invalid="ignore"):
            s = r.below_llik - r.above_llik
        assert np.array_equal(np.isnan(s), ids == CC.ZERO_NAN)
        assert np.array_equal(np.isneginf(s), ids == CC.ZERO_NINF)
        assert np.array_equal(np.isposinf(s), ids == CC.ZERO_PINF)


# ---------------------------------------------------------------------------
# e. the prefix decision on rare ties
# ---------------------------------------------------------------------------
def test_prefix_decision_on_rare_ties(engine):
    """16 keys of the rare-tie history in one launch, 2^20 candidates each:
    the prefix-first records are the full-stream ones byte for byte; a job
    stays open exactly when its prefix holds neither tied category -- one that
    holds one of them is decided, the other only ties -- and the winners of
    the open jobs lie past the prefix."""
    jobs = list(CC.rare_jobs())
    score = CC.job_scores(jobs[0])
    full, cdfs, none = _run(engine, jobs, 0)
    pre, cdfs_p, need = _run(engine, jobs, CC.PREFIX)
    assert none is None and need is not None
    assert [_rec(r) for r in pre] == [_rec(r) for r in full]
    # the device's own prefix streams: the same keys at one prefix of candidates
    heads, hcdfs, _ = _run(engine, [j._replace(n_cand=CC.PREFIX) for j in jobs], 0, outputs=True)
    count, late = [0, 0, 0], 0
    for i, (j, r) in enumerate(zip(jobs, pre)):
        assert np.array_equal(cdfs[i], cdfs_p[i]) and np.array_equal(cdfs[i], hcdfs[i])
        kp = heads[i].cand.astype(np.int64)
        assert np.array_equal(kp, CC.draw(cdfs[i], j.key, 0, CC.PREFIX))
        sit = CC.situation(kp)
        count[sit] += 1
        assert need[i] == CC.need_flag(kp, score, cdfs[i], j.n_cand) == int(sit == 0), (j.name, sit)
        first = CC.first_of(cdfs[i], j.key, 0, j.n_cand, CC.RARE_CATS)
        k1 = int(CC.draw(cdfs[i], j.key, first, 1)[0])
        assert (r.index, int(r.value), r.n_scored) == (first, k1, j.n_cand), (j.name, r, first)
        assert (r.index >= CC.PREFIX) == (sit == 0)
        assert np.float64(r.score).tobytes() == np.float64(pre[0].score).tobytes()
        late += int(r.index >= CC.PREFIX)
    print("rare tie: %d jobs with neither tied category in the prefix, %d with one, %d with both; "
          "%d winners past the prefix" % (count[0], count[1], count[2], late))
    assert min(count) >= 2 and late >= 1
