"""The lattice cases (tests/lattice_cases.py) are what they are named for,
shown with the oracle and the numpy replay of the streams (oracle/streams.py)
alone: the route each case takes, the winners past the prefix of the
rare-winner cases, the margins that make "index == argmax" a fair exact
assertion, the tie counts of the rounding mixtures and the clamp's streams.
tests/test_gpu_lattice_stages.py runs the kernels on the same table.
"""
import numpy as np
import pytest

from hyperopt_amd import engine as E
from tests import lattice_cases as LC


def test_case_table():
    assert len(set(LC.IDS)) == len(LC.CASES)
    assert len({c.key for c in LC.CASES}) == len(LC.CASES)
    assert LC.N_FULL == 3 * LC.TILE + 77 and LC.PREFIX == 4096
    assert E._lat_prefix(str(LC.PREFIX)) == LC.PREFIX      # the engine accepts it,
    with pytest.raises(ValueError):
        E._lat_prefix(str(LC.PREFIX // 2))                 # and nothing smaller
    for c in LC.CASES:
        assert c.n_cand == LC.N_FULL and c.n_cand < 1 << 15
        assert c.below.size + c.above.size < 5000
        q = c.args[2]
        for o in (c.below, c.above):
            assert np.all(np.isfinite(o)) and np.all(np.rint(o / q) * q == o), c.name
    # the routes the issue lists
    draws = {c.draw for c in LC.CASES}
    assert draws == {"pow2", "gen32", "gen64"}
    assert {c.kind for c in LC.CASES if c.draw == "gen32"} == {"quniform", "qnormal",
                                                               "qloguniform"}
    assert LC.lattice(LC.case("quniform(-3,7,0.25)"))[0] < 0       # negative kmin on POW2
    assert LC.lattice(LC.case("qnormal(0,10,3)"))[0] < -1          # unbounded, negative slots
    assert LC.case("quniform(1e6,1e6+100,1)").path == "prefix"     # fp64 draws, small lattice
    fams = {(LC.spec(c)[0], LC.spec(c)[4] is not None) for c in LC.RARE}
    assert fams == {("GMM1", True), ("GMM1", False), ("LGMM1", True), ("LGMM1", False)}


@pytest.mark.parametrize("c", LC.CASES, ids=LC.IDS)
def test_route(c):
    """draw, path and variant follow from the engine's rules (DRAW32_MAX_SLOT,
    LAT_SUGGEST_MAX_SLOTS) and the kernels' (lattice_pow2, qlpdf_big)."""
    assert LC.route(c) == (c.draw, c.path, c.variant)
    kmin, n = LC.lattice(c)
    fb, fa = LC.fits(c)
    if c.variant == "block":
        assert fa[0].size > LC.K_QBIG and fb[0].size <= LC.K_QBIG
    else:
        assert max(fa[0].size, fb[0].size) <= LC.K_QBIG
        assert 250 <= fa[0].size <= 350
    if c.draw == "pow2":
        assert n <= LC.K_LAT_LDS
    assert n <= E.LATTICE_CAP


def test_wide_lattices():
    for name in ("quniform(0,6000,1)", "quniform(0,6000,1)/block"):
        c = LC.case(name)
        kmin, n = LC.lattice(c)
        assert n > LC.K_LAT_LDS
        s = LC.replay_premise(c)["slots"]
        hi, lo = int(np.sum(s >= LC.K_LAT_LDS)), int(np.sum(s < LC.K_LAT_LDS))
        print("%s: %d drawn slots at or above %d, %d below" % (name, hi, LC.K_LAT_LDS, lo))
        assert hi >= 50 and lo >= 50
    for name in ("qlognormal(0,1,0.5)", "qlognormal(0,1,0.5)/block"):
        c = LC.case(name)
        kmin, n = LC.lattice(c)
        seen = LC.replay_premise(c)["slots"].size
        print("%s: %d slots, %d drawn" % (name, n, seen))
        assert n > E.LAT_PACK_MAX and n > 5e4      # the memset route; about 10^5 slots
        assert seen < n // 100                     # most unseen


@pytest.mark.parametrize("c", LC.CASES, ids=LC.IDS)
def test_winner_margin(c):
    """The oracle's winner of the replayed stream leads the runner-up value by
    more than the oracle's own rounding noise (scale_cases.oracle_noise) and
    than the kernels' pinned distance from the oracle."""
    p = LC.replay_premise(c)
    nz = LC.noise(c, p["values"])
    print("%s: winner %d, margin %.3g, oracle noise %.3g, fair above %.3g, %d ambiguous draws"
          % (c.name, p["winner"], p["margin"], nz, LC.fair_margin(p), p["ambiguous"]))
    assert p["margin"] > 100.0 * nz
    assert p["margin"] > 10.0 * LC.fair_margin(p)
    assert p["ambiguous"] <= 0.01 * c.n_cand     # stream_cases.CAP_Q


def test_rare_winners_lie_past_the_prefix():
    branches = set()
    for c in LC.RARE:
        p = LC.replay_premise(c)
        print("%s: winner at %d, %d late values, best of them %.3g above the prefix's best"
              % (c.name, p["winner"], p["late"].size, p["late_margin"]))
        assert p["late"].size >= 1 and p["winner"] >= LC.PREFIX, c.name
        assert p["late_margin"] > 10.0 * LC.fair_margin(p), c.name
        branches.add("fp64" if c.draw == "gen64" else "fp32")
    assert branches == {"fp32", "fp64"}


def test_settled_cases_have_no_late_value():
    assert len(LC.SETTLED) >= 6
    for c in LC.SETTLED:
        p = LC.replay_premise(c)
        assert p["late"].size == 0 and p["winner"] < LC.PREFIX, c.name


@pytest.mark.parametrize("name", sorted(LC.LEVELS))
def test_levels_mix(name):
    jobs = LC.level(name)
    assert 4 <= len(jobs) <= 6
    assert any(c.rare and c.n_cand > LC.PREFIX for c in jobs)
    assert any(not c.rare and c.n_cand > LC.PREFIX for c in jobs)
    assert any(c.n_cand <= LC.PREFIX for c in jobs)
    for c in jobs:
        if not c.rare and c.n_cand > LC.PREFIX:
            assert c.path == "compact" or LC.replay_premise(c)["late"].size == 0
    draws = {c.draw for c in jobs}
    if name == "pow2":
        assert draws == {"pow2"}
    if name == "gen32":
        assert draws == {"pow2", "gen32"}
    if name == "gen64":
        assert "gen64" in draws and draws != {"gen64"}
    if name == "block":
        assert {c.variant for c in jobs} == {"wave", "block"}
    # every rare family wins late in some level
    fams = {(LC.spec(c)[0], LC.spec(c)[4] is not None)
            for lv in LC.LEVELS for c in LC.level(lv) if c.rare}
    assert len(fams) == 4


@pytest.mark.parametrize("q", LC.TIE_Q)
def test_tie_streams_reach_the_redo_branch(q):
    """Draws of the tie mixtures within REDO |t| of a half-integer (the
    sampler's redo of the division), per stream; positive for every q that is
    not a power of two."""
    mu, sigma, w, kmin, n = LC.tie_mixture(q)
    assert np.all((mu / q - 0.5) == np.rint(mu / q - 0.5)) or not LC.is_pow2(q)
    for fp32 in (True, False):
        v = LC.tie_stream(q, LC.TIE_KEY, LC.N_FULL, fp32)
        k = np.rint(v / q)
        assert k.min() >= kmin and k.max() < kmin + n
        cnt = LC.redo_count(v, q)
        print("q = %g, %s stream: %d of %d draws in the redo window"
              % (q, "fp32" if fp32 else "fp64", cnt, v.size))
        if not LC.is_pow2(q):
            assert cnt > 0
        if fp32:
            assert cnt == v.size   # sigma below half an fp32 ulp: every draw is its mean
    # the tight fp64 stream: the mean or a double next to it, nearly all in the
    # window, and for some q many that the multiplication alone would misplace
    v = LC.tie_stream(q, LC.TIE_KEY, LC.N_FULL, False, rel=LC.TIE_TIGHT)
    cnt, dif = LC.redo_count(v, q), LC.differ_count(v, q)
    print("q = %g, tight fp64 stream: %d in the redo window, %d where v * (1 / q) and v / q "
          "round apart" % (q, cnt, dif))
    assert cnt > 0.9 * v.size
    assert (dif > 100) if q in LC.TIE_DIFFER_Q else (dif >= 0)


@pytest.mark.parametrize("fp32", [True, False], ids=["fp32", "fp64"])
@pytest.mark.parametrize("side", ["low", "high"])
def test_clamp_streams(side, fp32):
    slot = LC.clamp_slot(side)
    k, cl = LC.clamp_stream(side, LC.CLAMP_KEYS[side, fp32], LC.N_FULL, fp32)
    assert cl.all() and np.all(k == slot)
    k, cl = LC.clamp_stream(side, LC.CLAMP_KEYS[side, fp32], LC.N_FULL, fp32, inside=True)
    ins = np.flatnonzero(~cl)
    assert np.all(k[cl] == slot)
    assert ins.size >= 1 and ins[0] >= LC.PREFIX       # first drawn past the prefix
    for wins in (True, False):
        s = LC.clamp_scores(side, wins)
        assert np.isnan(s[0]) and np.isnan(s[-1]) and np.all(np.isfinite(s[1:-1]))
        better = s[k[ins] - LC.CLAMP_KMIN] > s[slot - LC.CLAMP_KMIN]
        print("%s, %s, inside %s: inside draws %s on slots %s, clamp slot %d, better %s"
              % (side, "fp32" if fp32 else "fp64", "wins" if wins else "loses", ins, k[ins],
                 slot, better))
        assert better.all() if wins else not better.any()
