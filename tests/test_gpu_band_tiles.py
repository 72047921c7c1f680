"""What the fast table scorer hands the band: the band tiles of
k_score_table_fast (tpe_table_score.hip) read back after a level.

Every tile's header {lo, hi_max, n} and entries {index, y, hi} are checked
against the kernel's own per-candidate scores and bounds (the table_scores
hook: the HOOKS=true instantiation) and the exact fp64 scores of the same
candidates, for the production instantiation (HOOKS=false: what tpe.suggest
runs) and the hook's alike; then the band theorem on those buffers, the
route k_band took (BandWork.{ns, direct, over}, offsets and thresholds from
tpe_band_layout) and the level's result.
"""
import numpy as np
import pytest

from tests import band_util as B
from tests.band_util import CONT

pytestmark = pytest.mark.gpu

N_CANDS = (1, 255, 8191, 8192, 8193, 3 * 8192 + 5)
BASES = (0, 3, 2 ** 32 - 2050)
HISTS = (3, 40, 2000)


@pytest.fixture(scope="module")
def engines():
    from hyperopt_amd.engine import Engine
    eng, eng64 = Engine(), Engine()
    eng64.exact64 = "dense"
    return eng, eng64


def _check_level(engines, works, tile_cap=None):
    """Run ``works`` (one table launch) with and without the per-candidate
    hooks and check every tile of both runs; returns per job what the partial
    overflow cases need."""
    import hyperopt_amd.engine as E
    eng, eng64 = engines
    K = B.layout()
    cap = E.BAND_TILE_CAP if tile_cap is None else tile_cap
    assert cap <= K.kTileSlots
    nj, nt = len(works), B.n_tiles_of([w.n_cand for w in works])
    hooked = eng.run(works, precision=32, scorer="table", table_scores=True)
    hdr_h, band_h = B.read_tiles(eng, nj, nt)
    work_h = B.read_work(eng, nj)
    over0 = eng.band_overflows
    prod = eng.run(works, precision=32, scorer="table")
    n_over = eng.band_overflows - over0
    hdr, band = B.read_tiles(eng, nj, nt)
    work = B.read_work(eng, nj)
    part = eng._bufs["partial"][:32 * nj * nt].cpu().numpy().view(B.L.BEST_DTYPE).reshape(nj, nt)
    assert eng.last_table_stats is not None  # the table path ran
    out, want_over = [], 0
    for j, (w, hk, r) in enumerate(zip(works, hooked, prod)):
        n, base = int(w.n_cand), int(w.cand_base)
        score, eps, cand = hk.extra["score"], hk.extra["eps"], hk.cand
        tab = hk.extra["table"]
        s64, best = B.dense64(eng64, w.kind, w.args, w.obs_below, w.obs_above, cand)
        with np.errstate(invalid="ignore"):
            hi_all = (score + eps).astype(np.float32)  # +inf: a log-sum-exp candidate
        ea = float(tab["eps_cubic"]) + 2.0001 * float(tab["eps_mix"])
        lo, hi_max, cnt = hdr["lo"][j], hdr["hi_max"][j], hdr["n"][j]
        # 1. the two instantiations: identical headers ...
        for k in ("lo", "hi_max", "n"):
            np.testing.assert_array_equal(hdr[k][j].view(np.uint32), hdr_h[k][j].view(np.uint32),
                                          err_msg="header %s, job %d" % (k, j))
        G = np.float32(lo.max())
        n_surv, surv_idx, full_matters, n_full = 0, [], False, 0
        for t in range(nt):
            a, b = t * K.kTileF, min(n, (t + 1) * K.kTileF)
            msg = "job %d tile %d" % (j, t)
            if a >= n:  # 2. a tile past the job's end
                assert lo[t] == -np.inf and hi_max[t] == -np.inf and cnt[t] == 0, msg
                assert part["index"][j, t] < 0, msg  # (empty_best: no candidate)
                continue
            # 2. the header's bounds hold for the exact scores
            assert lo[t] <= s64[a:b].max() <= hi_max[t], (msg, lo[t], s64[a:b].max(), hi_max[t])
            must = np.flatnonzero(~(hi_all[a:b] < lo[t])) + a
            # (the kernel's s >= s_thr has slack: whatever it adds has hi within
            # 2^-20 |lo| + 1e-4 (eps_cubic + 2.0001 eps_mix) below lo; twice that here)
            slack = 2.0 ** -19 * abs(float(lo[t])) + 1e-3 * ea + 1e-29
            may = np.flatnonzero(~(hi_all[a:b].astype(np.float64) < float(lo[t]) - slack)) + a
            if cnt[t] == K.kTileFull:  # 5. more than tile_cap: no entries to read
                n_full += 1
                assert may.size > cap, (msg, may.size, cap)
                full_matters |= not hi_max[t] < G
                continue
            assert cnt[t] <= cap, (msg, cnt[t], cap)
            e, e_h = (np.sort(x[j, t, :cnt[t]], order="index") for x in (band, band_h))
            # 1. ... and identical entry sets (their order in the tile is free)
            np.testing.assert_array_equal(e.view(np.uint8), e_h.view(np.uint8), err_msg=msg)
            # 3. the entries
            loc = e["index"] - base
            assert np.all(np.diff(loc) > 0) and loc.size == cnt[t], msg
            assert loc.size == 0 or (loc[0] >= a and loc[-1] < b), (msg, loc[:1], loc[-1:], a, b)
            B.assert_value_is(cand[loc], e["y"], w.kind)
            np.testing.assert_array_equal(e["hi"], hi_all[loc], err_msg=msg)
            assert np.all(e["hi"] >= s64[loc]), msg
            # 4. complete; extras only within the scorer's slack; 5. the count
            assert np.all(np.isin(must, loc)), (msg, np.setdiff1d(must, loc)[:5])
            assert np.all(np.isin(loc, may)), (msg, np.setdiff1d(loc, may)[:5])
            if not hi_max[t] < G:
                keep = ~(e["hi"] < G)
                n_surv += int(keep.sum())
                surv_idx.append(loc[keep])
        # 6. the band theorem on these buffers, the route and the result
        assert r.index == base + best and r.value == cand[best] and r.n_scored == n, \
            (r.index - base, best, s64[r.index - base], s64[best])
        for W in (work[j], work_h[j]):
            if full_matters:
                assert W["over"] == 1
            else:
                assert best in np.concatenate(surv_idx), (j, best)
                assert W["ns"] == n_surv and W["over"] in (0, 1)
                assert W["direct"] == int(n_surv <= K.kBandDirect)
                assert W["over"] == 0 or not W["direct"]
        if not (full_matters or work[j]["over"]):
            np.testing.assert_allclose(r.score, s64[best], rtol=1e-12, atol=1e-12)
            assert hk.score == r.score and hk.index == r.index
        want_over += int(full_matters or work[j]["over"])
        out.append(dict(n_full=n_full, n_tiles=-(-n // K.kTileF), full_matters=full_matters,
                        over=work[j]["over"]))
    assert n_over == want_over
    return out


def _work(kind, args, n_hist, n_cand, base, seed=0):
    from hyperopt_amd.engine import LabelWork
    below, above = B.history(kind, args, n_hist, 7000 + 13 * n_hist + seed)
    return LabelWork(kind, kind, args, below, above, n_cand=n_cand, cand_base=base,
                     key=0xBA2D0000 + 977 * n_hist + n_cand + seed)


def _cases():
    """Every (kind, n_cand) pair and every (kind, history) pair, the other
    axes cycled so that each value of each meets each kind."""
    out = []
    for ki, (kind, args) in enumerate(CONT):
        for ni, n in enumerate(N_CANDS):
            out.append((kind, args, HISTS[(ki + ni) % 3], n, BASES[(2 * ki + ni) % 3]))
        for hi, h in enumerate(HISTS):
            c = (kind, args, h, N_CANDS[-1], BASES[(ki + hi + 1) % 3])
            if c not in out:
                out.append(c)
    return out


@pytest.mark.parametrize("kind,args,n_hist,n_cand,base", _cases())
def test_band_tiles(engines, kind, args, n_hist, n_cand, base):
    """Natural histories (3 and 40 trials: wide cells, so two-polynomial and
    log-sum-exp candidates with hi = +inf), tile-boundary candidate counts,
    candidate indices across 2^32."""
    _check_level(engines, [_work(kind, args, n_hist, n_cand, base)])


@pytest.mark.parametrize("base", [0, 2 ** 32 - 2050])
def test_band_tiles_bounded_label_past_the_retry_list(engines, base):
    """About half of the below mass outside the bounds: waves whose
    rejections overflow the retry list (test_gpu_streams) -- the entries' y,
    drawn again by redraw, are still the stream's."""
    from hyperopt_amd.engine import LabelWork
    rng = np.random.RandomState(50)
    below, above = rng.uniform(0.0, 0.02, 25), rng.uniform(0.0, 10.0, 200)
    w = LabelWork("x", "uniform", (0.0, 10.0), below, above, n_cand=3 * 8192 + 5,
                  key=0x7E57_0000_0000_0032, cand_base=base)
    _check_level(engines, [w])


@pytest.mark.parametrize("kind,args", [CONT[0], CONT[3]])
def test_band_tiles_non_lean_sampler(engines, kind, args):
    """A below mixture past the scorer's LDS staging (explicit lists: 100
    below observations, 101 components): the one-candidate-at-a-time draw32
    branch of k_score_table_fast and of its redraw."""
    from hyperopt_amd.engine import LabelWork
    from tests.test_gpu_parity import _mixture_case
    g = _mixture_case(np.random.RandomState(11), kind, args, 100, 700, 1)
    w = LabelWork(kind, kind, args, g.obs_below, g.obs_above, n_cand=8193, cand_base=3,
                  key=0x4E0_1EA4)
    _check_level(engines, [w])
    eng = engines[0]
    fast, = eng.run([w], precision=32, scorer="table", table_scores=True)
    s, = eng.run([w], precision=32, sample_only=True)
    np.testing.assert_array_equal(fast.cand, s.cand)


def test_band_tiles_unequal_n_cand(engines):
    """Three labels in one launch with 4, 1 and 1 tiles of candidates: the
    launch's tiles past a job's end are empty."""
    works = [_work(kind, args, 2000, n, base, seed=j) for j, ((kind, args), n, base) in
             enumerate(zip((CONT[0], CONT[1], CONT[2]), (3 * 8192 + 5, 100, 8192),
                           (3, 0, 2 ** 32 - 2050)))]
    res = _check_level(engines, works)
    assert [r["n_tiles"] for r in res] == [4, 1, 1]


# (kind, BAND_TILE_CAP, history / key seed): a tile of a natural history holds
# its candidates within ~1e-5 of its best -- mostly one -- so the seeds are
# those whose tiles hold (1, 2, 1, 1), (1, 1, 2, 1), (16, 9, 15, 1), (2, 7, 11, 1)
# and (28, 20, 18, 1) such candidates; with (1, 1, 2, 1) the full tile cannot
# hold the winner
PARTIAL = [(0, 1, 2), (0, 1, 6), (0, 8, 5), (1, 1, 2), (1, 1, 6), (1, 8, 5), (2, 1, 2), (2, 8, 0),
           (3, 1, 2), (3, 8, 0)]


@pytest.mark.parametrize("ki,cap,seed", PARTIAL)
def test_band_tiles_partial_overflow(engines, ki, cap, seed, monkeypatch):
    """BAND_TILE_CAP shrunk so that some tiles of a 3-trial history overflow
    and some do not: a full tile makes the level re-score the label exactly
    only when it can hold the winner (hi_max >= G; _check_level compares
    band_overflows), and the winner is the exact argmax either way."""
    import hyperopt_amd.engine as E
    monkeypatch.setattr(E, "BAND_TILE_CAP", cap)
    kind, args = CONT[ki]
    res, = _check_level(engines, [_work(kind, args, 3, 3 * 8192 + 5, 0, seed=seed)])
    assert 1 <= res["n_full"] < res["n_tiles"], res
    if seed == 6:
        assert not res["full_matters"] and not res["over"]
