"""The quantized lattice path (csrc/tpe_quantized.hip) stage by stage, on the
cases of tests/lattice_cases.py (whose premises tests/test_lattice_cases.py
proves on the CPU): the first-index table slot by slot, the compaction, the
slot scores, the prefix-first decision with its conditional second pass, the
clamp's slot and the off-lattice guard -- through direct calls of the five
exports (tests/lattice_util.py) and through Engine.run.

The reference stream is tpe_sample's at the job's own draw precision
(tests/test_gpu_streams.py pins it to the numpy replay): cand = rint(v / q) q,
k = rint(cand / q).  Every comparison is exact unless it says otherwise.
"""
import numpy as np
import pytest

from hyperopt_amd import _lib as L
from tests import lattice_cases as LC
from tests import lattice_util as U

pytestmark = pytest.mark.gpu

PREFIX_CASES = [c for c in LC.CASES if c.path == "prefix"]
_cache = {}


def _solo(c):
    """One Level of the case alone at N_FULL, base 0 (shared by the tests)."""
    if ("solo", c.name) not in _cache:
        lv = U.Level([U.job_spec(c)])
        _cache["solo", c.name] = (lv, lv.own_streams()[0])
    return _cache["solo", c.name]


def _lattice_index(cand, q):
    k = np.rint(cand / q).astype(np.int64)
    assert np.all(k.astype(np.float64) * q == cand)   # every candidate is a lattice value
    return k


def _same_bits(a, b):
    """Equal as bits, NaNs as NaNs (whatever their payload)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(U.bits(a)[~np.isnan(a)], U.bits(b)[~np.isnan(b)])


# ---------------------------------------------------------------------------
# a. the first-index table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", LC.CASES, ids=LC.IDS)
def test_first_index_table(c):
    """slot_first after tpe_lattice_sample, every slot: cand_base + the first
    occurrence of (kmin + s) q in the stream, all-ones where the value does not
    occur; sentinels intact, no error bit.  Eight jobs per case -- n_cand 1,
    100, one tile, three tiles and 77, each at base 0 and at an odd shard base
    past 2^32 -- every one launched alone with the caller's all-ones fill
    (TPE_F_LATTICE_READY), then all together with the library's memset."""
    specs = [U.job_spec(c, n_cand=n, cand_base=b) for b in (0, LC.BASE_ODD) for n in LC.N_ODD]
    lv = U.Level(specs)
    streams = lv.own_streams()
    want = []
    for sp, cand in zip(specs, streams):
        assert cand.size == sp["n_cand"]
        t, off = U.expected_table(cand, sp["q"], sp["kmin"], sp["slots"], sp["cand_base"])
        assert off == 0
        want.append(t)
    assert np.array_equal(streams[3][:100], streams[1])      # one stream per (key, base)
    empty = [np.full(sp["slots"], U.ONES, np.uint64) for sp in specs]
    for j in range(len(specs)):
        tables, ok = lv.sample(ready=True, only=[j])
        assert ok and lv.err() == 0, (c.name, j)
        for i, t in enumerate(tables):
            bad = np.flatnonzero(t != (want[j] if i == j else empty[i]))
            assert bad.size == 0, (c.name, j, i, bad[:5], t[bad[:5]], want[j][bad[:5]])
    tables, ok = lv.sample(ready=False)
    assert ok and lv.err() == 0
    for j, t in enumerate(tables):
        bad = np.flatnonzero(t != want[j])
        assert bad.size == 0, (c.name, j, bad[:5], t[bad[:5]], want[j][bad[:5]])
    if c.name.startswith("quniform(0,6000"):
        seen = np.flatnonzero(want[3] != U.ONES)
        assert np.sum(seen >= LC.K_LAT_LDS) >= 50 and np.sum(seen < LC.K_LAT_LDS) >= 50


# ---------------------------------------------------------------------------
# b. the kernel choice does not change the table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pow2,other", [("quniform(0,100,1)", "quniform(0,100,3)"),
                                         ("quniform(-3,7,0.25)", "quniform(0,10,0.1)"),
                                         ("rare:qloguniform(2,6,1)", "qloguniform(0,4,3)"),
                                         ("rare:qnormal(0,10,0.25)", "quniform(1e6,1e6+100,1)")])
def test_pow2_job_on_the_general_kernel(pow2, other):
    """A pow2 job alone runs k_lattice_sample<POW2> (slots from rintf in
    fp32); beside a non-pow2 (or fp64) job the launch runs the general
    instantiation (`mark` in fp64 on the same fp32 draws).  The same table,
    bit for bit -- the stream's."""
    a, b = LC.case(pow2), LC.case(other)
    assert a.draw == "pow2" and b.draw != "pow2"
    lv = U.Level([U.job_spec(a), U.job_spec(b)])
    cand = lv.own_streams()
    want = [U.expected_table(x, sp["q"], sp["kmin"], sp["slots"], 0)[0]
            for x, sp in zip(cand, lv.specs)]
    alone, ok = lv.sample(ready=True, only=[0])
    assert ok and lv.err() == 0
    both, ok = lv.sample(ready=True)
    assert ok and lv.err() == 0
    assert np.array_equal(alone[0], both[0])
    assert np.array_equal(both[0], want[0]) and np.array_equal(both[1], want[1])


def test_mixed_launch_equals_solo_tables():
    """Four jobs of one launch with n_cand 1, 100, one tile and three tiles
    and 77, mixed kinds, lattices below and above kLatLds slots: each job's
    table is the table of the job launched alone."""
    names = ("quniform(0,100,1)", "quniform(0,6000,1)", "qnormal(0,10,3)", "qlognormal(0,1,0.5)")
    specs = [U.job_spec(LC.case(nm), n_cand=n) for nm, n in zip(names, LC.N_ODD)]
    assert min(sp["slots"] for sp in specs) < LC.K_LAT_LDS < max(sp["slots"] for sp in specs)
    lv = U.Level(specs)
    solo = []
    for j in range(len(specs)):
        tables, ok = lv.sample(ready=True, only=[j])
        assert ok and lv.err() == 0
        solo.append(tables[j])
    for ready in (True, False):
        tables, ok = lv.sample(ready=ready)
        assert ok and lv.err() == 0
        for j, sp in enumerate(specs):
            assert np.array_equal(tables[j], solo[j]), (names[j], ready)
            assert np.sum(solo[j] != U.ONES) >= 1
    cand = lv.own_streams()
    for j, sp in enumerate(specs):
        assert np.array_equal(solo[j], U.expected_table(cand[j], sp["q"], sp["kmin"],
                                                        sp["slots"], 0)[0])


# ---------------------------------------------------------------------------
# c. rounding ties
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fp32", [True, False], ids=["fp32", "fp64"])
@pytest.mark.parametrize("q", LC.TIE_Q)
def test_rounding_ties(q, fp32):
    """Components at (k + 1/2) q with sigmas of 1e-12 |mu| (and, third run,
    2e-16 |mu|: the mean or a double next to it): every draw sits on a
    rounding tie or next to it.  The table puts each draw on rint(v / q) of
    tpe_sample's value, although the sampler multiplies by 1 / q and divides
    only inside the tie window -- which the streams reach (counted here on the
    device's unquantized draws, on the replay in test_lattice_cases.py).  On
    the tight fp64 stream the multiplication alone would misplace hundreds of
    draws at q = 0.1 and q = 3."""
    for base, rel in ((0, LC.TIE_REL_SIGMA), (LC.BASE_ODD, LC.TIE_REL_SIGMA), (0, LC.TIE_TIGHT)):
        mu, sigma, w, kmin, n = LC.tie_mixture(q, rel)
        mix = (w, mu, sigma)
        lv = U.Level([U.mixture_spec("tie", mix, mix, None, None, q, LC.TIE_KEY, LC.N_FULL, kmin,
                                     n, fp32, cand_base=base)])
        prec = 32 if fp32 else 64
        cand = lv.stream(prec)[0]
        v = lv.stream(prec, quantized=False)[0]
        assert np.array_equal(np.rint(v / q) * q, cand)
        redo, dif = LC.redo_count(v, q), LC.differ_count(v, q)
        print("q = %g, %s, base %d, sigma %g |mu|: %d of %d draws in the redo window, %d where "
              "v * (1 / q) and v / q round apart, %d distinct values"
              % (q, "fp32" if fp32 else "fp64", base, rel, redo, v.size, dif,
                 np.unique(cand).size))
        if not LC.is_pow2(q):
            assert redo > 0
        if rel == LC.TIE_TIGHT and not fp32 and q in LC.TIE_DIFFER_Q:
            assert dif > 100   # the redo branch decides these draws
        want, off = U.expected_table(cand, q, kmin, n, base)
        assert off == 0
        for ready in (True, False):
            tables, ok = lv.sample(ready=ready)
            assert ok and lv.err() == 0
            bad = np.flatnonzero(tables[0] != want)
            assert bad.size == 0, (q, fp32, bad + kmin, tables[0][bad], want[bad])


# ---------------------------------------------------------------------------
# d. compaction
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", LC.CASES, ids=LC.IDS)
def test_compaction(c):
    """counts[j] = the number of distinct stream values; the (value, first
    index) pairs are np.unique's of the stream, values as bits -- (double) k *
    q, so +0.0 for k = 0 where the stream's rint(v / q) * q may hold -0.0 --
    in any order (the kernel appends by atomic)."""
    lv, cand = _solo(c)
    q = c.args[2]
    k = _lattice_index(cand, q)
    u, f = np.unique(k, return_index=True)
    for ready in (True, False):
        lv.sample(ready=ready)
        (vals, firsts), = lv.compact(ready=ready)
        assert vals.size == u.size
        o = np.argsort(firsts, kind="stable")
        ow = np.argsort(f, kind="stable")
        assert np.array_equal(firsts[o], f[ow])
        assert np.array_equal(U.bits(vals[o]), U.bits(u[ow].astype(np.float64) * q))
    if LC.lattice(c)[0] < -1:
        assert (u < 0).any()          # negative values took part


# ---------------------------------------------------------------------------
# e. slot scores equal value scores
# ---------------------------------------------------------------------------
def _check_slot_scores(lv, names):
    by_reach = {}
    for reach in (True, False):
        r = lv.suggest(reach=reach)
        assert r["sentinels"] and lv.err() == 0       # (slots below 0 raise no error bit)
        inj, _ = lv.score_values([lv.slot_values(j) for j in range(lv.nj)], reach=reach)
        lv.sample()
        lv.compact()
        comp, _ = lv.score_compacted(reach=reach)
        for j in range(lv.nj):
            J, P = lv.jobs[j], r["partial"][j]
            vals = lv.slot_values(j)
            assert np.array_equal(U.bits(P["value"]), U.bits(vals)), names[j]
            assert np.all(P["index"] == -1)
            # score_slots against k_score_q on the injected slot values
            assert _same_bits(P["score"], inj[j][2]), (names[j], reach)
            with np.errstate(invalid="ignore"):
                assert _same_bits(inj[j][0] - inj[j][1], inj[j][2])
            # ... and against k_score_q on the compacted (drawn) values
            s = np.rint(comp[j]["value"] / J["q"]).astype(np.int64) - int(J["lat_kmin"])
            assert s.size >= 1 and np.all((s >= 0) & (s < J["lat_n"]))
            assert _same_bits(comp[j]["score"], P["score"][s]), (names[j], reach)
            assert not np.any(np.isnan(comp[j]["score"]))
        by_reach[reach] = (r, inj)
    for j in range(lv.nj):   # the component windows do not change a bit
        assert _same_bits(by_reach[True][0]["partial"][j]["score"],
                          by_reach[False][0]["partial"][j]["score"])
    return by_reach[True]


@pytest.mark.parametrize("c", PREFIX_CASES, ids=[c.name for c in PREFIX_CASES])
def test_slot_scores(c):
    """partial[s] of score_slots (read after tpe_lattice_suggest) against
    tpe_score_quantized on the injected values (kmin + s) q and on the
    compacted drawn values: the same bits, NaNs as NaNs, with the reach
    arrays and without (every kernel scoring a value forms the
    same bits).  Against the oracle the finite log-masses agree within
    test_gpu_mixture's 1e-8 (1 + |lpdf|) per side; the two bracket slots of a
    bounded lattice score NaN."""
    lv, _ = _solo(c)
    r, inj = _check_slot_scores(lv, [c.name])
    vals, score = lv.slot_values(0), r["partial"][0]["score"]
    bl, al = inj[0][0], inj[0][1]
    ok = vals >= 0 if LC.spec(c)[0] == "LGMM1" else np.ones(vals.size, bool)
    _, ref = LC.oracle_scores(c, vals[ok])
    for dev, key in ((bl[ok], "below_llik"), (al[ok], "above_llik")):
        want = ref[key]
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(dev), fin), c.name
        assert np.all(np.abs(dev[fin] - want[fin]) <= 1e-8 * (1.0 + np.abs(want[fin]))), c.name
    if LC.spec(c)[4] is not None:   # bounded: the brackets (and no drawn slot beside them)
        assert np.isnan(score[0]) and np.isnan(score[-1])
        table = lv.sample()[0][0]
        assert np.all(table[np.isnan(score)] == U.ONES)


def test_slot_scores_wave_beside_block():
    """One score_slots / k_score_q grid with wave-variant and block-variant
    jobs: every job's slot scores are those of the job alone."""
    jobs = LC.level("block")
    lv = U.Level([U.job_spec(c) for c in jobs])
    r, _ = _check_slot_scores(lv, [c.name for c in jobs])
    for j, c in enumerate(jobs):
        solo, _ = _solo(LC.case(c.name))
        alone = solo.suggest()["partial"][0]
        assert _same_bits(alone["score"], r["partial"][j]["score"]), c.name


# ---------------------------------------------------------------------------
# f. the decision and the second pass
# ---------------------------------------------------------------------------
def _decision(name, ready=False):
    """(level jobs, Level, tpe_lattice_suggest's results, the full-stream
    best records, streams, premises) of a lattice_cases level, cached."""
    if ("dec", name, ready) not in _cache:
        jobs = LC.level(name)
        lv = U.Level([U.job_spec(c) for c in jobs])
        r = lv.suggest(prefix=LC.PREFIX, ready=ready)
        err = lv.err()
        full = lv.full_stream_best(ready=ready)
        cand = lv.own_streams()
        prem = [LC.premise(c, _lattice_index(x, c.args[2])) for c, x in zip(jobs, cand)]
        _cache["dec", name, ready] = (jobs, lv, r, err, full, cand, prem)
    return _cache["dec", name, ready]


@pytest.mark.parametrize("ready", [False, True], ids=["memset", "ready"])
@pytest.mark.parametrize("name", sorted(LC.LEVELS))
def test_prefix_decision(name, ready):
    """tpe_lattice_suggest at the smallest prefix on a launch that mixes
    rare-winner jobs, settled ones and one of at most a prefix of candidates:
    the full-stream records byte for byte, np.argmax of the oracle's scores
    over the job's own stream, and the need flags the CPU premises call for --
    some set, some clear, so the second pass's tile loop both runs and skips."""
    jobs, lv, r, err, full, cand, prem = _decision(name, ready)
    assert err == 0 and r["sentinels"]
    for j, c in enumerate(jobs):
        b = r["best"][j]
        assert b.tobytes() == full[j].tobytes(), (c.name, b, full[j])
        p = prem[j]
        assert p["margin"] > LC.fair_margin(p)
        assert b["index"] == p["winner"], (c.name, b, p["winner"])
        assert b["n_scored"] == c.n_cand and b["value"] == cand[j][p["winner"]]
        assert abs(b["score"] - p["score"].max()) <= 2e-8 * (1.0 + p["lpdf"])
        if c.n_cand <= LC.PREFIX:
            assert r["need"][j] == 0, c.name
        if p["late"].size:
            assert r["need"][j] == 1, c.name
        if c.rare and c.n_cand > LC.PREFIX:    # the device's stream keeps the CPU's premise
            assert p["late"].size >= 1 and p["winner"] >= LC.PREFIX, c.name
        # the table after the second pass: the whole stream of a job that
        # needed it, the prefix alone of one that did not
        n = c.n_cand if r["need"][j] else min(c.n_cand, LC.PREFIX)
        want, off = U.expected_table(cand[j][:n], c.args[2], int(lv.jobs[j]["lat_kmin"]),
                                     int(lv.jobs[j]["lat_n"]), 0)
        assert off == 0 and np.array_equal(r["tables"][j], want), c.name
    assert (r["need"] == 0).any() and (r["need"] == 1).any()


def test_every_rare_family_wins_past_the_prefix():
    fams = set()
    for name in sorted(LC.LEVELS):
        jobs, lv, r, err, full, cand, prem = _decision(name)
        for j, c in enumerate(jobs):
            if c.rare and r["best"][j]["index"] >= LC.PREFIX:
                fams.add((LC.spec(c)[0], LC.spec(c)[4] is not None))
    assert fams == {("GMM1", True), ("GMM1", False), ("LGMM1", True), ("LGMM1", False)}


@pytest.fixture(scope="module")
def engine():
    from hyperopt_amd.engine import Engine
    return Engine()


def _works(jobs):
    from hyperopt_amd.engine import LabelWork
    return [LabelWork("q%d" % i, c.kind, c.args, c.below, c.above, n_cand=c.n_cand, key=c.key)
            for i, c in enumerate(jobs)]


def _engine_streams(engine, works, flags):
    s32 = engine.run(works, precision=32, sample_only=True)
    s64 = engine.run(works, precision=64, sample_only=True)
    return [(a if f & L.F_DRAW32 else b).cand for a, b, f in zip(s32, s64, flags)]


def _tuple(r):
    return (r.score, r.index, r.value, r.n_scored)


@pytest.mark.parametrize("name", sorted(LC.LEVELS))
def test_engine_levels(engine, name):
    """The same levels through Engine.run with engine.lat_prefix = 4096 and
    with 0 (every stream drawn in full): equal results, the oracle's argmax
    over the own stream; a wide lattice added to the level moves the slice to
    sample -> compact -> score and changes nobody else's result."""
    jobs = LC.level(name)
    works = _works(jobs)
    old = engine.lat_prefix
    out = {}
    try:
        for p in (LC.PREFIX, 0):
            engine.lat_prefix = p
            out[p] = [_tuple(r) for r in engine.run(works, precision=32)]
            flags = engine.last_plan[3]["flags"].copy()
        wide = LC.case("quniform(0,6000,1)")
        engine.lat_prefix = LC.PREFIX
        more = [_tuple(r) for r in engine.run(works + _works([wide]), precision=32)]
    finally:
        engine.lat_prefix = old
    assert out[LC.PREFIX] == out[0]
    assert more[:len(jobs)] == out[0]
    for c, f in zip(jobs, flags):
        assert bool(f & L.F_DRAW32) == (c.draw != "gen64"), c.name
    cand = _engine_streams(engine, works, flags)
    for c, x, res in zip(jobs, cand, out[0]):
        p = LC.premise(c, _lattice_index(x, c.args[2]))
        assert p["margin"] > LC.fair_margin(p)
        assert res[1] == p["winner"] and res[2] == x[p["winner"]] and res[3] == c.n_cand, c.name
    # the added wide job is the one test_wide_lattice_winner checks alone
    s, = engine.run(_works([wide]), precision=64, sample_only=True)
    p = LC.premise(wide, _lattice_index(s.cand, 1.0))
    assert more[-1][1] == p["winner"]


# ---------------------------------------------------------------------------
# g. the clamp's slot
# ---------------------------------------------------------------------------
def _clamp_level(side, fp32, inside, wins, base=0):
    b = LC.clamp_mixture(side, inside)
    a = LC.clamp_above(side, wins)
    return U.Level([U.mixture_spec("clamp", (b[2], b[0], b[1]), (a[2], a[0], a[1]), LC.CLAMP_LOW,
                                   LC.CLAMP_HIGH, LC.CLAMP_Q, LC.CLAMP_KEYS[side, fp32],
                                   LC.N_FULL, LC.CLAMP_KMIN, LC.CLAMP_SLOTS, fp32,
                                   cand_base=base)])


@pytest.mark.parametrize("fp32", [True, False], ids=["fp32", "fp64"])
@pytest.mark.parametrize("side", ["low", "high"])
def test_clamp_slot(side, fp32):
    """Every component far outside the bounds: every attempt is rejected and
    the last one clamped, the stream is one value -- the slot whose bin holds
    the bound, first seen at cand_base, returned without a second pass.  With
    a component of weight 1.2e-6 inside the bounds a value first drawn after
    the prefix is found when it scores higher (need set) and loses when it
    does not."""
    slot = LC.clamp_slot(side)
    base = LC.BASE_ODD
    lv = _clamp_level(side, fp32, False, True, base)
    cand, = lv.own_streams()
    assert np.all(cand == slot * LC.CLAMP_Q)
    want = np.full(LC.CLAMP_SLOTS, U.ONES, np.uint64)
    want[slot - LC.CLAMP_KMIN] = base
    tables, ok = lv.sample()
    assert ok and lv.err() == 0 and np.array_equal(tables[0], want)
    r = lv.suggest()
    assert lv.err() == 0 and r["sentinels"]
    b = r["best"][0]
    assert r["need"][0] == 0 and b["index"] == base and b["value"] == slot * LC.CLAMP_Q
    assert b["n_scored"] == LC.N_FULL and np.array_equal(r["tables"][0], want)
    for wins in (True, False):
        lv = _clamp_level(side, fp32, True, wins)
        cand, = lv.own_streams()
        k = _lattice_index(cand, LC.CLAMP_Q)
        ins = np.flatnonzero(k != slot)
        assert ins.size >= 1 and ins[0] >= LC.PREFIX
        s = LC.clamp_scores(side, wins)
        sc = s[k - LC.CLAMP_KMIN]
        winner = int(np.argmax(sc))
        assert (winner >= LC.PREFIX) == wins
        r = lv.suggest()
        assert lv.err() == 0 and r["sentinels"]
        b = r["best"][0]
        assert b.tobytes() == lv.full_stream_best()[0].tobytes()
        assert b["index"] == winner and b["value"] == cand[winner], (side, fp32, wins, b)
        assert abs(b["score"] - sc[winner]) <= 2e-8 * (1.0 + abs(sc[winner]))
        assert r["need"][0] == (1 if wins else 0)


# ---------------------------------------------------------------------------
# h. the off-lattice guard
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quniform(0,100,1)", "quniform(0,100,3)",
                                  "quniform(1e6,1e6+100,1)", "qnormal(0,10,3)"])
def test_off_lattice_guard(name):
    """A job whose declared lattice covers the lower half of the support only
    (every buffer as large as declared): error bit 2, no word outside the
    job's slots changed, the slots inside correct."""
    c = LC.case(name)
    kmin, n = LC.lattice(c)
    half = n // 2
    lv = U.Level([U.job_spec(c, lattice=(kmin, half))])
    cand, = lv.own_streams()
    want, off = U.expected_table(cand, c.args[2], kmin, half, 0)
    assert off > 100 and np.sum(want != U.ONES) > 5
    for ready in (True, False):
        tables, ok = lv.sample(ready=ready)
        assert lv.err() & 2
        assert ok
        assert np.array_equal(tables[0], want)


# ---------------------------------------------------------------------------
# i. the winner on the wide lattices, through the engine
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("c", LC.WIDE, ids=[c.name for c in LC.WIDE])
def test_wide_lattice_winner(engine, c, precision):
    works = _works([c])
    timers = {}
    r, = engine.run(works, precision=precision, timers=timers)
    assert "lat" in timers
    assert not engine.last_plan[3]["flags"][0] & L.F_DRAW32
    kmin, n = LC.lattice(c)
    from hyperopt_amd.engine import LAT_PACK_MAX
    memset = n > LAT_PACK_MAX
    hj = engine.last_plan[3][:1].copy()
    assert bool(hj["flags"][0] & L.F_LATTICE_READY) == (not memset)
    if memset:   # (else the slots live in the level's upload block)
        (slot, vals, firsts), = U.read_engine(engine, hj)
    s, = engine.run(works, precision=64, sample_only=True)
    p = LC.premise(c, _lattice_index(s.cand, c.args[2]))
    assert p["margin"] > LC.fair_margin(p)
    assert r.index == p["winner"] and r.value == s.cand[r.index] and r.n_scored == c.n_cand
    np.testing.assert_allclose(r.score, p["score"].max(), rtol=1e-9, atol=1e-12)
    if memset:   # the engine's own table and compaction of this level
        assert np.array_equal(slot, U.expected_table(s.cand, c.args[2], kmin, n, 0)[0])
        u, f = np.unique(_lattice_index(s.cand, c.args[2]), return_index=True)
        assert np.array_equal(np.sort(firsts), np.sort(f)) and vals.size == u.size
