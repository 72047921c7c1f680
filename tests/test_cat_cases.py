"""The categorical cases (tests/cat_cases.py) are what they are named for,
shown with the oracle and the numpy replay of the streams (oracle/streams.py)
alone: which K tell numpy's pairwise sum from its leaf and from a sequential
sum, the 8192-element buffer rule of np.sum, the bit-equal tied scores, the
NaN / +inf / -inf pattern of zero prior probabilities, the three situations of
the rare tie and the kernel variants and sampler regimes of the mixed launches.
tests/test_gpu_categorical.py runs the kernels on the same table.
"""
import numpy as np
import pytest

from tests import cat_cases as CC
from tests import settings_cases as SC


def test_case_table():
    assert CC.SETTINGS[0] == (25, 1.0)
    assert CC.SETTINGS[1][0] in SC.COUNT_LF and CC.SETTINGS[1][1] in SC.COUNT_PW
    assert set(CC.DISCRIMINATING_K) >= {200, 300, 1000}
    assert set(CC.DISCRIMINATING_K) <= set(CC.POSTERIOR_K) and CC.CHUNK_K in CC.POSTERIOR_K
    assert {1, 7, 8, 9, 127, 128, 129, 136, 200, 300, 1000, 4097, 8192, 8193, 10000} <= \
        set(CC.POSTERIOR_K)
    assert max(CC.HIST_K) == 1000 and min(CC.HIST_K) > 32
    for K in CC.POSTERIOR_K:
        for kind in CC.KINDS:
            args, below, above = CC.posterior_case(K, kind)
            assert below.size == 25 and 3000 <= above.size == max(3 * K, 3000) <= 30_000
            assert 0 <= min(below.min(), above.min()) and max(below.max(), above.max()) < K
    keys = [j.key for name in CC.LEVELS for j in CC.level(name)] + list(CC.TIE_KEYS) + \
        list(CC.ZERO_KEYS) + list(CC.RARE_KEYS)
    assert len(set(keys)) == len(keys)
    assert CC.RARE_N == 1 << 20 and CC.PREFIX == 4096 and len(CC.RARE_KEYS) == 16


def _pseudo(K):
    for kind in CC.KINDS:
        args, below, above = CC.posterior_case(K, kind)
        for lf, pw in CC.SETTINGS:
            for side, obs in (("below", below), ("above", above)):
                ps = CC.pseudocounts(kind, args, obs, pw, lf)
                # the array the oracle sums
                assert np.array_equal(ps / np.sum(ps), CC.posterior(kind, args, obs, pw, lf))
                yield (kind, lf, pw, side), ps


@pytest.mark.parametrize("K", [K for K in CC.POSTERIOR_K if K <= CC.NP_BUF])
def test_pairwise_restatement_is_np_sum(K):
    """np_pw_leaf / np_pairwise_sum restated in Python: np.sum bit for bit up
    to one buffer."""
    for what, ps in _pseudo(K):
        assert CC.pairwise(ps) == np.sum(ps), (K, what)
        assert CC.chunked(ps) == np.sum(ps), (K, what)


@pytest.mark.parametrize("K", CC.DISCRIMINATING_K)
def test_discriminating_k(K):
    """A total from the leaf alone, and a sequential one, each change bits of
    the above posterior -- of either kind, under either setting."""
    for (kind, lf, pw, side), ps in _pseudo(K):
        leaf, seq = CC.bits_changed(ps, CC.pw_leaf(ps)), CC.bits_changed(ps, CC.sequential(ps))
        print("K = %d %s lf=%d pw=%g %s: %d of %d entries change with the leaf-only total, %d "
              "with the sequential one" % (K, kind, lf, pw, side, leaf, K, seq))
        if side == "above":
            assert leaf >= 1 and seq >= 1, (K, kind, lf, pw)


@pytest.mark.parametrize("K", [K for K in CC.POSTERIOR_K if K > CC.NP_BUF])
def test_np_sum_goes_buffer_by_buffer(K):
    """Past 8192 doubles np.sum is the sequential sum of the pairwise sums of
    the consecutive 8192-element chunks; at CHUNK_K that is not the pairwise
    sum of the whole array (the total the kernel formed before)."""
    differ = 0
    for what, ps in _pseudo(K):
        assert CC.chunked(ps) == np.sum(ps), (K, what, np.__version__)
        whole = CC.pairwise(ps)
        differ += int(whole != np.sum(ps) and CC.bits_changed(ps, whole) > 0)
    print("K = %d: %d of 8 posteriors change bits under the whole-array pairwise sum (numpy %s)"
          % (K, differ, np.__version__))
    if K == CC.CHUNK_K:
        assert differ >= 4
        ps = dict(_pseudo(K))["randint", 25, 1.0, "above"]
        assert CC.bits_changed(ps, CC.pairwise(ps)) > 0   # the default settings, too


def test_tie_case():
    """Categories 0 and 5: the same bits in both posteriors and in the score,
    the maximum, of below mass 1/33; category 5 comes first under some keys."""
    j = CC.tie_jobs(CC.TIE_N[0])[0]
    pb, pa = CC.job_posteriors(j)
    s = CC.job_scores(j)
    a, b = CC.TIE_CATS
    assert pb[a].tobytes() == pb[b].tobytes() and pa[a].tobytes() == pa[b].tobytes()
    assert s[a].tobytes() == s[b].tobytes() and pb[a] == 1.0 / 33.0
    assert np.all(np.delete(s, CC.TIE_CATS) < s[a] - 1.0) and not np.isnan(s).any()
    later = 0
    for n in CC.TIE_N:
        for j in CC.tie_jobs(n):
            cdf = CC.oracle_cdf(j)
            r = CC.replay(j, cdf, s)
            fa, fb = (int(np.flatnonzero(r["k"] == c)[0]) for c in CC.TIE_CATS)   # both occur
            assert r["index"] == min(fa, fb) and r["value"] == (a if fa < fb else b)
            assert max(fa, fb) < CC.PREFIX and r["need"] == 0
            later += int(fb < fa and n == CC.TIE_N[0])
    print("category %d drawn before category %d under %d of %d keys" % (b, a, later,
                                                                       len(CC.TIE_KEYS)))
    assert later >= 2 and len(CC.TIE_KEYS) - later >= 2


def test_zero_probability_case():
    """p = (0.3, 0, 0.3, 0, 0.4, 0): category 1 scores NaN, 3 +inf, 5 -inf, the
    others finite.  Neither category 1 nor category 5 takes a word: thr[5] ==
    thr[4], both saturated at 2^32 - 1, and the one word below no threshold,
    2^32 - 1, belongs to category 4, the last one with mass (a rule "the last
    category up to 2^32" would hand it to category 5)."""
    j = CC.zero_job()
    pb, pa = CC.job_posteriors(j)
    s = CC.job_scores(j)
    assert np.isnan(s[CC.ZERO_NAN]) and s[CC.ZERO_PINF] == np.inf and s[CC.ZERO_NINF] == -np.inf
    assert np.all(np.isfinite(s[[0, 2, 4]]))
    assert pb[CC.ZERO_NAN] == 0.0 == pa[CC.ZERO_NAN] and pb[CC.ZERO_NINF] == 0.0 == pa[CC.ZERO_PINF]
    assert pb[CC.ZERO_PINF] > 0.1                      # +inf is drawable
    cdf = CC.oracle_cdf(j)
    lo, hi = CC.intervals(cdf)
    thr = CC.S.thresholds(cdf)
    assert hi[CC.ZERO_NAN] == lo[CC.ZERO_NAN] and hi[CC.ZERO_NINF] == lo[CC.ZERO_NINF]
    assert thr[CC.ZERO_NINF] == thr[CC.ZERO_NINF - 1] == 2 ** 32 - 1
    assert int(hi[4]) == 2 ** 32 and lo[0] == 0 and np.array_equal(lo[1:], hi[:-1])  # a partition
    assert hi[CC.ZERO_PINF] - lo[CC.ZERO_PINF] > 2 ** 28
    # the words at the edges land where the intervals say, the last word included
    words = np.array([0, int(hi[0]) - 1, int(hi[0]), int(lo[4]), 2 ** 32 - 2, 2 ** 32 - 1])
    ks = CC.S.categorical_of_word(cdf, words)
    assert ks.tolist() == [0, 0, 2, 4, 4, 4]
    assert np.all((lo[ks] <= words.astype(np.uint64)) & (words.astype(np.uint64) < hi[ks]))
    for key in CC.ZERO_KEYS:
        for n, base in ((1001, 0), (CC.TILE * 16 + 3, 3), (1 << 17, 0)):
            r = CC.replay(j._replace(key=key, n_cand=n, cand_base=base), cdf, s)
            assert not np.isin(r["k"], (CC.ZERO_NAN, CC.ZERO_NINF)).any()
            assert r["value"] == CC.ZERO_PINF and r["score"] == np.inf and r["need"] == 0
            assert r["index"] == base + int(np.flatnonzero(r["k"] == CC.ZERO_PINF)[0])
    # the injected ids: np.argmax takes the first NaN, else the first +inf
    inj = np.array(CC.ZERO_INJ)
    assert int(np.argmax(s[inj])) == 6 and inj[6] == CC.ZERO_NAN
    assert int(np.argmax(s[inj[inj != CC.ZERO_NAN]])) == 3
    # the need rule does not reopen a job for the undrawable NaN category, and
    # would for a drawable one
    kp = CC.draw(cdf, CC.ZERO_KEYS[0], 0, CC.PREFIX)
    assert CC.need_flag(kp, s, cdf, 1 << 17) == 0
    flat = np.cumsum(np.full(6, 1.0 / 6.0))
    assert CC.need_flag(kp, s, flat, 1 << 17) == 1 and CC.need_flag(kp, s, flat, CC.PREFIX) == 0
    # the last category scoring NaN: still no word, still no reason to go on
    jl = CC.zero_job(last_nan=True)
    sl = CC.job_scores(jl)
    assert np.isnan(sl[[CC.ZERO_NAN, 5]]).all() and sl[CC.ZERO_PINF] == np.inf
    cl = CC.oracle_cdf(jl)
    assert np.array_equal(cl, cdf)                     # the same below posterior
    assert CC.need_flag(kp, sl, cl, 1 << 17) == 0


def test_rare_tie_case():
    """Two categories of prior p = 1.03e-3 and no observation: bit-equal best
    scores of below mass 2e-4.  Over the 16 keys a prefix of 4096 candidates
    holds neither (the job stays open and its winner lies past the prefix),
    exactly one, or both (the job is decided: the unseen one only ties)."""
    jobs = CC.rare_jobs()
    pb, pa = CC.job_posteriors(jobs[0])
    s = CC.job_scores(jobs[0])
    a, b = CC.RARE_CATS
    assert pb[a].tobytes() == pb[b].tobytes() and s[a].tobytes() == s[b].tobytes()
    assert 1.9e-4 < pb[a] < 2.1e-4 and np.all(s[:4] < s[a] - 1.0)
    cdf = CC.oracle_cdf(jobs[0])
    lo, hi = CC.intervals(cdf)
    assert np.all(hi > lo)
    count, late = [0, 0, 0], 0
    for j in jobs:
        kp = CC.draw(cdf, j.key, 0, CC.PREFIX)
        sit = CC.situation(kp)
        count[sit] += 1
        need = CC.need_flag(kp, s, cdf, j.n_cand)
        first = CC.first_of(cdf, j.key, 0, j.n_cand, CC.RARE_CATS)
        assert need == int(sit == 0) and first >= 0
        assert (first >= CC.PREFIX) == (sit == 0)
        late += int(first >= CC.PREFIX)
    print("rare tie: %d jobs with neither tied category in the prefix, %d with one, %d with both; "
          "%d winners past the prefix" % (count[0], count[1], count[2], late))
    assert min(count) >= 2 and late >= 1


def test_mixed_launches_cover_variants_and_regimes():
    variants, regimes, under = set(), set(), {}
    for name, ks in CC.LEVELS.items():
        kr = CC.variant(ks)
        variants.add(kr)
        for K in ks:
            regimes.add(CC.regime(K, kr))
            under.setdefault(K, set()).add(kr)
        jobs = CC.level(name)
        assert {j.n_cand for j in jobs} == set(CC.N_MIXED)
        assert {j.cand_base for j in jobs} == set(CC.BASE_MIXED)
    assert variants == set(CC.KR) and regimes == {"regs", "search", "plain"}
    assert {CC.regime(K, 16) for K in CC.LEVELS["all"]} == {"regs", "search", "plain"}
    assert under[3] == {4, 8, 16} and under[2] == {4, 16} and under[8] == {8, 16}
    assert CC.variant((CC.TIE_K,)) == 8 and CC.variant(CC.LEVELS["all"] + (CC.TIE_K,)) == 16


@pytest.mark.parametrize("name", sorted(CC.LEVELS))
def test_mixed_jobs_have_a_fair_winner(name):
    """"index == np.argmax of the oracle's scores" is a fair exact assertion:
    the categories of the best score hold the same pair of posterior entries
    (the same score bits on any implementation), every other category scores
    lower by far more than a log's rounding, and the stream draws one of the
    best."""
    for j in CC.level(name):
        pb, pa = CC.job_posteriors(j)
        s = CC.job_scores(j)
        assert not np.isnan(s).any()
        top = np.flatnonzero(s == s.max())
        assert np.all(pb[top] == pb[top[0]]) and np.all(pa[top] == pa[top[0]]), j.name
        assert np.all(np.delete(s, top) < s.max() - 1e-9), j.name
        for n in (j.n_cand, CC.N_PREFIXED):
            r = CC.replay(j._replace(n_cand=n), CC.oracle_cdf(j), s)
            assert r["value"] in top, (j.name, n)
