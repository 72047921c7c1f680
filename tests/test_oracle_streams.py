"""The numpy replay of the Philox streams (oracle/streams.py) checked on its
own, without a GPU: Random123's known answers for Philox4x32-10, the
extremes of the uniforms, the agreement of the two documented component
rules, the distributions the replay produces, and -- from the replay alone --
the caps on ambiguous candidates that tests/test_gpu_streams.py relies on."""
import numpy as np
import pytest
from scipy import stats

from oracle import streams as S
from oracle import tpe_oracle as O
from tests import stream_cases as C

N = 200_000
P_MIN = 1e-4  # the suite's threshold (test_gpu_sampler.py)


def _words(s):
    return [int(x, 16) for x in s.split()]


# ---------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000",
     "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff",
     "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0",
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    got = S.philox4x32(_words(ctr), _words(key))
    assert [int(x) for x in got] == _words(want)
    # the round count matters: nine rounds give other words
    assert [int(x) for x in S.philox4x32(_words(ctr), _words(key), rounds=9)] != _words(want)


def test_draw_words_counter_layout():
    """{idx lo, idx hi, attempt, stream} / {key lo, key hi}, vectorised."""
    key = 0xA4093822_299F31D0  # key lo = 299f31d0, hi = a4093822
    idx = np.array([0x05A308D3_243F6A88, 7, 2 ** 32 + 7], np.int64)
    got = S.draw_words(key, idx, 0x13198A2E, 0x03707344)
    want = S.philox4x32([0x243F6A88, 0x05A308D3, 0x13198A2E, 0x03707344],
                        [0x299F31D0, 0xA4093822])
    assert np.array_equal(got[0], want)
    assert not np.array_equal(got[1], got[2])  # the high index word reaches the counter
    neg = S.draw_words(key, -1, 0, S.SAMP)     # int64 -1: both index words all ones
    assert np.array_equal(neg, S.philox4x32([0xFFFFFFFF, 0xFFFFFFFF, 0, S.SAMP],
                                            [0x299F31D0, 0xA4093822]))
    assert len({S.SAMP, S.RETR, S.PRIO, S.ANNL}) == 4
    assert (S.SAMP, S.RETR, S.PRIO, S.ANNL) == tuple(
        int.from_bytes(s, "big") for s in (b"SAMP", b"RETR", b"PRIO", b"ANNL"))


def test_u01_extremes():
    top = 2 ** 32 - 1
    assert S.u01_f64(0, 0) == 0.0
    assert S.u01_f64(top, top) == 1.0 - 2.0 ** -53
    assert S.u01_f64(1 << 5, 0) == 2.0 ** -27 and S.u01_f64(0, 1 << 6) == 2.0 ** -53
    assert S.u01_f64(31, 63) == 0.0  # the low 5 / 6 bits are dropped
    assert S.u01_f32(0) == 0.0 and S.u01_f32(top) == 1.0 - 2.0 ** -24 and S.u01_f32(255) == 0.0


def test_cos_turns_is_exact_at_the_zeros():
    c = np.array([0, 1 << 30, 1 << 31, 3 << 30, (1 << 30) + 1, (1 << 30) - 1], np.uint64)
    got = S.cos_turns32(c)
    assert got[0] == 1.0 and got[1] == 0.0 and got[2] == -1.0 and got[3] == 0.0
    # one step past / before the zero: -+ sin(2 pi 2^-32), to the last bit
    step = np.sin(2.0 * np.pi * 2.0 ** -32)
    assert got[4] == -step and got[5] == step
    rnd = np.random.RandomState(0).randint(0, 2 ** 32, 10_000, dtype=np.uint64)
    np.testing.assert_allclose(S.cos_turns32(rnd), np.cos(2 * np.pi * rnd / 2.0 ** 32),
                               rtol=0, atol=1e-15)  # the naive form rounds its angle


# ---------------------------------------------------------------------------
# component rules
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CASES, ids=C.CASE_IDS)
def test_component_rules_agree(c):
    """first k with cdf[k] > w 2^-32 cdf[-1]  ==  first k with w < thr[k], for
    every word within +-2 of every threshold and 1e5 random words."""
    cdf, _, _ = C.host_cdf(c)
    thr = S.thresholds(cdf)
    near = (thr.astype(np.int64)[:, None] + np.arange(-2, 3)[None, :]).reshape(-1)
    near = near[(near >= 0) & (near < 2 ** 32)]
    rnd = np.random.RandomState(len(cdf)).randint(0, 2 ** 32, 100_000, dtype=np.uint64)
    w = np.concatenate([near.astype(np.uint64), rnd, [0, 2 ** 32 - 1]]).astype(np.uint64)
    a, b = S.component_cdf(cdf, w), S.component_thr(thr, w)
    assert np.array_equal(a, b), (w[a != b][:5], a[a != b][:5], b[a != b][:5])
    # residuals: in (0, 1], and the two forms agree to the grid's resolution
    k = a
    t_thr, t_cdf = S.residual_thr(thr, k, w), S.residual_cdf(cdf, k, w)
    wide = (thr[k] - np.where(k > 0, thr[np.maximum(k - 1, 0)], 0)) > (1 << 16)
    last = k == len(cdf) - 1  # the last threshold is saturated at 2^32 - 1
    sel = wide & ~last
    assert np.all((t_thr[sel] > 0) & (t_thr[sel] <= 1))
    assert np.all((t_cdf > 0) & (t_cdf <= 1))
    np.testing.assert_allclose(t_thr[sel], t_cdf[sel], rtol=0, atol=2.0 ** -15)


def test_multi_case_has_multi_buckets():
    cdf, _, _ = C.host_cdf(C.case("multi"))
    assert C.multi_buckets(cdf) >= 3


# ---------------------------------------------------------------------------
# distributions of the replay
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform-25", "normal-25", "loguniform-25", "half"])
@pytest.mark.parametrize("precision", [64, 32])
def test_replay_ks(name, precision):
    c = C.case(name)
    cdf, mu, sig = C.host_cdf(c)
    draw = S.gmm_draw64 if precision == 64 else S.gmm_draw32
    rep = draw(cdf, mu, sig, c.key, np.arange(N), c.low, c.high)
    y = rep["y"]
    if c.low is not None:
        assert y.min() >= c.low and y.max() < c.high
    w = np.diff(np.concatenate([[0.0], cdf]))
    p = stats.kstest(y, lambda v: O.truncated_mixture_cdf(v, w, mu, sig, c.low, c.high)).pvalue
    assert p > P_MIN, p
    # the normals alone: standard normal before truncation (unbounded case)
    if c.low is None:
        assert stats.kstest(rep["z"], "norm").pvalue > P_MIN


@pytest.mark.parametrize("K", [3, 40, 300])
def test_replay_categorical_chi2(K):
    p = np.random.RandomState(K).dirichlet(np.full(K, 2.0))
    cdf = np.cumsum(p)
    k = S.categorical_draw(cdf, 0xC0FFEE + K, np.arange(N))
    assert k.min() >= 0 and k.max() < K
    counts = np.bincount(k, minlength=K)
    expect = p / cdf[-1] * N
    keep = expect >= 20
    obs_c = np.append(counts[keep], counts[~keep].sum())
    exp_c = np.append(expect[keep], expect[~keep].sum())
    if exp_c[-1] == 0:
        obs_c, exp_c = obs_c[:-1], exp_c[:-1]
    assert stats.chisquare(obs_c, exp_c)[1] > P_MIN


def test_replay_anneal_pick_is_geometric():
    g, _ = S.anneal_pick(0xABCDEF0123, np.arange(N), 2.0, 10 ** 6)
    top = 12
    counts = np.bincount(np.minimum(g, top), minlength=top + 1)
    p = 0.5 ** (np.arange(top + 1) + 1.0)   # P(geometric(1/2) - 1 = g)
    p[top] = 0.5 ** top                      # the tail
    assert stats.chisquare(counts, p * N)[1] > P_MIN
    # clipped to the rows there are; p >= 1 always picks the best row
    g3, _ = S.anneal_pick(0xABCDEF0123, np.arange(1000), 1000.0, 3)
    assert g3.max() == 2 and g3.min() >= 0
    assert np.all(S.anneal_pick(5, np.arange(100), 1.0, 7)[0] == 0)
    # the pick and the value use separate counters
    assert not np.array_equal(S.draw_words(5, 9, 0, S.ANNL), S.draw_words(5, 9, 1, S.ANNL))


def test_replay_priors_follow_their_formulas():
    rec = dict(kind=S.PRIOR_UNIFORM, n_cat=0, a=0.0, b=1.0, q=0.0, p_off=0)
    idx = np.arange(2 ** 32 - 5, 2 ** 32 + 5)
    d = S.prior_draw(rec, None, 77, idx)
    r = S.draw_words(77, idx, 0, S.PRIO)
    assert np.array_equal(d["v"], S.u01_f64(r[:, 0], r[:, 1]))  # uniform(0, 1) is u itself
    assert len(set(d["v"])) == idx.size                          # no repeat across 2^32
    rec = dict(kind=S.PRIOR_CATEGORICAL, n_cat=3, a=0.0, b=0.0, q=0.0, p_off=1)
    k = S.prior_draw(rec, [9.0, 0.1, 0.3, 0.6], 78, np.arange(N))["v"]
    assert stats.chisquare(np.bincount(k.astype(int), minlength=3),
                           np.array([0.1, 0.3, 0.6]) * N)[1] > P_MIN


# ---------------------------------------------------------------------------
# the caps the GPU comparison relies on, from the replay alone
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def replays():
    cache = {}

    def get(name, precision, base):
        k = (name, precision, base)
        if k not in cache:
            c = C.case(name)
            cdf, mu, sig = C.host_cdf(c)
            draw = S.gmm_draw64 if precision == 64 else S.gmm_draw32
            cache[k] = draw(cdf, mu, sig, c.key, C.indices(c, base), c.low, c.high)
        return cache[k]
    return get


@pytest.mark.parametrize("c", C.CASES, ids=C.CASE_IDS)
def test_ambiguity_caps(c, replays):
    for base in C.BASES:
        r64, r32 = replays(c.name, 64, base), replays(c.name, 32, base)
        n64, n32 = int(C.ambiguous64(c, r64).sum()), int(C.ambiguous32(c, r32).sum())
        print("%s base=%d: ambiguous fp64 %d (cap %d), fp32 %d (cap %d)"
              % (c.name, base, n64, C.CAP64, n32, int(C.CAP32 * c.n)))
        assert n64 <= C.CAP64
        assert n32 <= C.CAP32 * c.n


def test_named_paths_are_reached(replays):
    """The rejection-heavy cases reach the paths they are named for, at every
    base: a wave with more rejections than its list holds; three or more
    retry calls; every attempt rejected and both clamps taken."""
    for base in C.BASES:
        assert C.max_wave_rejections(replays("half", 32, base)) > C.RETRY_LIST
        r97 = replays("r97", 32, base)
        assert r97["calls"].max() >= 3 and r97["rejected0"].mean() > 0.9
        for precision in (64, 32):
            rep = replays("clamp", precision, base)
            c = C.case("clamp")
            assert rep["clamped"].all()
            top = np.nextafter(c.high, -np.inf) if precision == 64 else \
                float(np.nextafter(np.float32(c.high), np.float32(-np.inf)))
            assert set(np.unique(rep["y"])) == {c.low, top}


@pytest.mark.parametrize("name,q", C.QUANT)
def test_quantized_ambiguity_caps(name, q, replays):
    c = C.case(name)
    for base in C.BASES[:2]:
        for precision in (64, 32):
            rep = replays(name, precision, base)
            cdf, mu, sig = C.host_cdf(c)
            tol = C.tol64(rep, mu, sig) if precision == 64 else C.tol32(rep, rep["y"])
            _, amb = C.quant_index(c, rep, q, tol, fast_exp=precision == 32)
            print("%s q=%g base=%d fp%d: half-integer ambiguous %d of %d"
                  % (name, q, base, precision, int(amb.sum()), c.n))
            assert amb.sum() <= C.CAP_Q * c.n


def test_prior_ambiguity_caps():
    labels, rec, pool = C.prior_records()
    assert len(labels) == 12 and len(set(rec["key"].tolist())) == 12
    for base in C.PRIOR_BASES:
        idx = base + np.arange(C.PRIOR_N, dtype=np.int64)
        for lab, R in zip(labels, rec):
            d = S.prior_draw(R, pool, int(R["key"]), idx)
            assert np.all(np.isfinite(d["v"]))
            if C.prior_is_smooth(R) and float(R["q"]) > 0:
                n = int(C.prior_half(R, d).sum())
                print("prior %s base=%d: half-integer ambiguous %d (cap %d)"
                      % (lab, base, n, C.CAP_PRIOR))
                assert n <= C.CAP_PRIOR


def test_anneal_ambiguity_cap():
    """No fixed trial id has a quotient log(u1) / log1p(-p) next to an integer."""
    losses, active, vals, keys = C.anneal_history()
    for avg in C.ANNEAL_AVG:
        for j in range(3):
            t = np.arange(j, C.ANNEAL_TRIALS, 3)
            g, quo = S.anneal_pick(int(keys[j]), C.ANNEAL_IDS[t], avg, int(active[:, j].sum()))
            assert not np.any(np.abs(quo - np.rint(quo)) <= C.ANNEAL_QUOTIENT_TOL)
            assert g.min() >= 0 and g.max() < active[:, j].sum()
