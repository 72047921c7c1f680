"""The band rescue (tpe_band_rescore: k_band, k_band_final, k_band_pick)
replayed on crafted band tiles, path by path.

A real level is run once (scorer="table"), so that the segments, fp64
coefficients and cell tables are the device's own; then crafted headers and
entries are copied over the engine's band buffers and the real
tpe_band_rescore is called again with the recorded pointers.  A crafted
tile's survivors have hi = +big, everything else hi below G; their y are
fp32 values of the test's choice.  Every case asserts the route the job took
(BandWork.{ns, ncell, over, direct} and the listed cells; offsets and every
threshold from tpe_band_layout) and the result against the oracle's
below_llik - above_llik at cand_value(y) and the dense fp64 kernel on the
same values -- not one score but a ranking: the winner is taken out of the
band and the job replayed, 32 times.

tpe_band_layout does not expose the per-chunk slow-component lists
(BandMix.n_dir): whether a case reached them, or a list's overflow exit to
the direct sum, is not asserted here.
"""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _lib as L
from tests import band_util as B
from tests.band_util import CONT
from tests.table_util import band_cell

pytestmark = pytest.mark.gpu

N_TILES = 24
N_PEEL = 32
G = np.float32(-1.25)  # the crafted jobs' best lower bound
BIG = np.float32(3e38)
HEAD = (0, 1, 0, 255, 3)  # the first tiles' entry counts
JS, TS, BS, ES = (d.itemsize for d in (L.JOB_DTYPE, L.TABLE_DTYPE, L.BEST_DTYPE, L.BAND_DTYPE))
MAXDIFF = {}  # path -> largest |score - dense|, |score - oracle| seen (printed at the end)


class _Lib(object):
    """The library, every call forwarded; tpe_band_rescore's arguments kept."""

    def __init__(self, lib):
        self._lib, self.args, self.host_jobs = lib, None, None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "tpe_band_rescore":
            return fn

        def call(*args):
            self.args = tuple(a.value if isinstance(a, ctypes.c_void_p) else a for a in args)
            self.host_jobs = np.frombuffer(ctypes.string_at(self.args[1], self.args[2] * JS),
                                           L.JOB_DTYPE).copy()
            return fn(*args)
        return call


class Setup(object):
    """One real level of ``kinds`` labels (n_tiles tiles of candidates each)
    on an engine of its own, and tpe_band_rescore replayed on its buffers."""

    def __init__(self, kinds, n_hist, n_tiles=N_TILES, table_cap=None):
        import torch
        import hyperopt_amd.engine as E
        self.torch, self.K = torch, B.layout()
        K = self.K
        eng = self.eng = E.Engine()
        eng.native = False  # the call is issued eagerly, and seen
        rec = eng.lib = _Lib(eng.lib)
        self.kinds, self.nt, self.n_cand = kinds, n_tiles, n_tiles * K.kTileF
        self.hist = [B.history(kind, args, n_hist, 9100 + n_hist + 7 * j)
                     for j, (kind, args) in enumerate(kinds)]
        works = [E.LabelWork("%s%d" % (kind, j), kind, args, below, above, n_cand=self.n_cand,
                             key=0xB7A9D + j)
                 for j, ((kind, args), (below, above)) in enumerate(zip(kinds, self.hist))]
        old = E.TABLE_CAP
        try:
            if table_cap is not None:
                E.TABLE_CAP = table_cap
            self.res = eng.run(works, precision=32, scorer="table")
        finally:
            E.TABLE_CAP = old
        self.stats = eng.last_table_stats
        assert rec.args is not None, "the level did not reach tpe_band_rescore"
        (self.dj, _, self.nj, self.d_segs, self.d_c64, self.d_tab, self.d_band, self.d_ctl,
         self.d_part, self.npart, _, self.d_work, self.sp) = rec.args
        self.hj = rec.host_jobs
        assert self.nj == len(kinds) and np.all(self.hj["n_cand"] == self.n_cand)
        assert (self.sp or 0) == torch.cuda.current_stream(eng.device).cuda_stream
        for name, p in (("band", self.d_band), ("band_ctl", self.d_ctl), ("band_work", self.d_work),
                        ("partial", self.d_part), ("tables", self.d_tab)):
            assert eng._bufs[name].data_ptr() == p, name
        assert self.npart >= self.nj * self.nt
        self.tables = eng._bufs["tables"][:TS * self.nj].cpu().numpy().view(L.TABLE_DTYPE).copy()

    def replay(self, crafted, j0=0, zero=True):
        """tpe_band_rescore on the crafted jobs (one Crafted per job, from job
        j0 on); returns (their tpe_best records, their routes)."""
        torch, K, eng = self.torch, self.K, self.eng
        nj, nt = len(crafted), self.nt
        assert 0 <= j0 and j0 + nj <= self.nj
        for name, arrs, per in (("band_ctl", [c.ctl for c in crafted], 4 * K.kHdrWords * nt),
                                ("band", [c.band for c in crafted], ES * K.kTileSlots * nt),
                                ("partial", [c.part for c in crafted], BS * nt)):
            raw = np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in arrs])
            assert raw.size == per * nj
            eng._bufs[name][per * j0:per * (j0 + nj)].copy_(torch.from_numpy(raw))
        if zero:
            eng._bufs["band_work"][K.work_bytes * j0:K.work_bytes * (j0 + nj)].zero_()
        best = torch.full((nj * BS,), 0xEE, dtype=torch.uint8, device=eng.device)
        hj = np.ascontiguousarray(self.hj[j0:j0 + nj])
        L.check(L.load().tpe_band_rescore(
            self.dj + JS * j0, hj.ctypes.data, nj, self.d_segs, self.d_c64, self.d_tab + TS * j0,
            self.d_band + ES * K.kTileSlots * nt * j0, self.d_ctl + 4 * K.kHdrWords * nt * j0,
            self.d_part + BS * nt * j0, nt * nj, best.data_ptr(), self.d_work + K.work_bytes * j0,
            self.sp), "tpe_band_rescore")
        torch.cuda.synchronize()
        return best.cpu().numpy().view(L.BEST_DTYPE).copy(), B.read_work(eng, self.nj)[j0:j0 + nj]


_setups = {}


def setup(kinds, n_hist, n_tiles=N_TILES, table_cap=None):
    key = (tuple(kinds), n_hist, n_tiles, table_cap)
    if key not in _setups:
        _setups[key] = Setup(list(kinds), n_hist, n_tiles, table_cap)
    return _setups[key]


@pytest.fixture(scope="module")
def eng64():
    from hyperopt_amd.engine import Engine
    e = Engine()
    e.exact64 = "dense"
    yield e
    _setups.clear()
    for path in sorted(MAXDIFF):
        print("band paths: %-28s max |score - dense fp64| %.3g (rel %.3g), |score - oracle| %.3g"
              % ((path,) + tuple(MAXDIFF[path])))


# ---------------------------------------------------------------------------
# the table's cells, as the kernels form them
# ---------------------------------------------------------------------------
def y_in_cells(tab, cells, rng):
    """One fp32 y per entry of ``cells``, well inside its cell (|u| <= 0.9)."""
    cells = np.asarray(cells, np.int64)
    u = rng.uniform(-0.9, 0.9, cells.size)
    y = (float(tab["origin"]) + (2 * cells + 1 + u) * float(tab["h"])).astype(np.float32)
    assert np.array_equal(band_cell(tab, y), cells)
    return y


def pick_cells(tab, n, rng):
    """n distinct cells of the table, its first and last among them."""
    nb = int(tab["nb"])
    assert nb >= n, "the table has %d cells, the case needs %d" % (nb, n)
    if n == 1:
        return np.array([rng.randint(nb)])
    inner = rng.choice(np.arange(1, nb - 1), n - 2, replace=False) if n > 2 else []
    return np.sort(np.concatenate([[0, nb - 1], inner]).astype(np.int64))


# ---------------------------------------------------------------------------
# crafted tiles
# ---------------------------------------------------------------------------
def counts_for(need, n_tiles, rng):
    """Entry counts per tile: HEAD, then full tiles, a partial one and empty
    ones, for at least ``need`` entries and some more."""
    K = B.layout()
    assert HEAD[3] == K.kTileSlots - 1 and n_tiles > len(HEAD) + 2
    counts, left = list(HEAD), need + 20 - sum(HEAD)
    for t in range(len(HEAD), n_tiles):
        c = int(min(max(left, 0), K.kTileSlots))
        if c == 0 and t % 3 == 0:
            c = int(rng.randint(1, 30))  # a tile of non-survivors alone
        counts.append(c)
        left -= c
    assert left <= 0, "%d entries do not fit %d tiles" % (need, n_tiles)
    return counts


class Crafted(object):
    """One job's crafted band tiles.  ``y``, ``idx``: the entries that can be
    survivors, in flat entry order; ``alive``: which of them are (hi = +big
    or +inf; the others and the filler have hi below G).  The filler entries
    have y = NaN: one that is scored wins."""

    def __init__(self, n_tiles, y, idx, alive, rng, counts=None, place=None):
        K = B.layout()
        self.y, self.idx = np.asarray(y, np.float32), np.asarray(idx, np.int64)
        self.alive = np.asarray(alive, bool).copy()
        n = self.y.size
        assert np.unique(self.idx).size == n
        counts = counts_for(n, n_tiles, rng) if counts is None else list(counts)
        assert len(counts) == n_tiles and max(counts) <= K.kTileSlots
        self.counts = np.asarray(counts)
        total = int(self.counts.sum())
        tile = np.repeat(np.arange(n_tiles), self.counts)
        slot = np.arange(total) - np.repeat(np.cumsum(self.counts) - self.counts, self.counts)
        pos = np.sort(rng.choice(total, n, replace=False)) if place is None else np.asarray(place)
        self.tile, self.slot = tile[pos], slot[pos]
        self.ctl = np.zeros((n_tiles, K.kHdrWords), np.uint32)
        self.band = np.zeros((n_tiles, K.kTileSlots), L.BAND_DTYPE)
        self.part = np.zeros(n_tiles, L.BEST_DTYPE)
        self.part["index"] = -1
        # stale entries past a tile's count, and the filler: NaN, the smallest indices
        self.band["y"], self.band["hi"] = np.nan, BIG
        self.band["index"] = 1 + np.arange(self.band.size).reshape(self.band.shape)
        low = np.array([np.nextafter(G, np.float32(-np.inf)), G - np.float32(1), -np.inf],
                       np.float32)
        for t in range(n_tiles):
            self.band["hi"][t, :counts[t]] = low[(t + np.arange(counts[t])) % 3]
        self.band["y"][self.tile, self.slot] = self.y
        self.band["index"][self.tile, self.slot] = self.idx
        # headers: G on one tile (an empty one if there is one), lower or -inf
        # elsewhere; hi_max +inf / +big over the tiles that hold these
        # entries, G (read, nothing kept) or below G (skipped) over the others
        lo = np.where(np.arange(n_tiles) % 2 == 0, G - rng.uniform(0.1, 5.0, n_tiles), -np.inf)
        empty = np.flatnonzero(self.counts == 0)
        lo[empty[-1] if empty.size else rng.randint(n_tiles)] = G
        mine = np.isin(np.arange(n_tiles), self.tile)
        hm = np.where(mine, np.where(np.arange(n_tiles) % 2 == 0, np.inf, BIG),
                      np.where(np.arange(n_tiles) % 4 < 2, G, G - np.float32(0.5)))
        self.ctl[:, 0] = lo.astype(np.float32).view(np.uint32)
        self.ctl[:, 1] = hm.astype(np.float32).view(np.uint32)
        self.ctl[:, 2] = self.counts
        # the entries k_band counts: those of the tiles it reads, in tile order
        self.read = ~(hm.astype(np.float32) < G) & (self.counts > 0)
        self.n_ent = int(self.counts[self.read].sum())
        self._write_hi()

    def _write_hi(self):
        k = np.arange(self.y.size)
        up = np.where(k % 5 == 0, np.float32(np.inf), np.where(k % 5 == 1, G, BIG))
        dn = np.where(k % 2 == 0, np.nextafter(G, np.float32(-np.inf)), -BIG)
        self.band["hi"][self.tile, self.slot] = np.where(self.alive, up, dn).astype(np.float32)

    def set_alive(self, k, on):
        self.alive[k] = on
        self._write_hi()

    def full(self, t, matters):
        """Tile t did not fit its entries; ``matters``: it can hold the winner."""
        assert not np.any(self.tile == t)
        self.ctl[t, 2] = B.layout().kTileFull
        self.ctl[t, 1] = np.float32(np.inf if matters else G - np.float32(0.25)).view(np.uint32)

    def partials(self, rng):
        """fp32 partials of the test's own; returns their np.argmax record."""
        n = self.part.size
        self.part["score"] = rng.normal(size=n).astype(np.float32)
        self.part["index"] = _indices(rng, n)
        self.part["value"] = rng.normal(size=n)
        self.part["index"][rng.randint(n)] = -1  # an empty one
        a, b = rng.choice(np.flatnonzero(self.part["index"] >= 0), 2, replace=False)
        self.part["score"][[a, b]] = 9.0  # the maximum twice: the smaller index
        k = a if self.part["index"][a] < self.part["index"][b] else b
        return float(self.part["score"][k]), int(self.part["index"][k]), \
            float(self.part["value"][k])


def rank_first(score, idx, alive):
    """np.argmax over the alive entries: NaN first, then the largest score,
    then the smallest index."""
    k = np.flatnonzero(alive)
    s = score[k]
    nan = np.isnan(s)
    if nan.any():
        k = k[nan]
    else:
        k = k[s == s.max()]
    return int(k[np.argmin(idx[k])])


def gap_ok(score, y, alive, first):
    """The reference separates the winner from every other alive entry that
    is not the same y: by more than 1e-9 max(1, |s|)."""
    k = np.flatnonzero(alive)
    k = k[(y[k].view(np.uint32) != y[first].view(np.uint32)) & ~np.isnan(y[k])]
    if np.isnan(score[first]) or k.size == 0:
        return True
    return bool(score[first] - np.nanmax(score[k]) > 1e-9 * max(1.0, abs(score[first])))


class Case(object):
    """A crafted job with its references: the oracle's and the dense fp64
    kernel's scores of every entry that can be a survivor."""

    def __init__(self, S, eng64, crafted, j=0, spare_of=None):
        self.S, self.j, self.c = S, j, crafted
        self.kind, self.args = S.kinds[j]
        below, above = S.hist[j]
        self.value = B.cand_value(crafted.y, self.kind)
        self.dense, _ = B.dense64(eng64, self.kind, self.args, below, above, self.value)
        self.oracle = B.oracle_scores(self.kind, self.args, below, above, self.value)
        # (copies of one y: one score, whatever lane of a vector loop computed it)
        _, first, inv = np.unique(crafted.y.view(np.uint32), return_index=True, return_inverse=True)
        self.dense, self.oracle = self.dense[first[inv]], self.oracle[first[inv]]
        fin = np.isfinite(self.oracle)
        assert np.array_equal(np.isnan(self.oracle), np.isnan(self.dense))
        # the two references agree (this project's bound, test_gpu_table.py)
        np.testing.assert_allclose(self.dense[fin], self.oracle[fin], rtol=1e-6, atol=1e-9)
        self.spare_of = spare_of  # entry -> the spares that may replace it (cells: its cell's)
        self.cell = band_cell(S.tables[j], crafted.y)

    def route(self):
        """(ns, ncell, direct, over, listed cells) the job must take."""
        K, a = self.S.K, self.c.alive
        ns = int(a.sum())
        cells = np.unique(self.cell[a])
        off = bool(np.any(cells < 0))
        cells = cells[cells >= 0]
        cells_ok = cells.size <= K.kBandCells and not off and ns <= K.kBandSurvMax
        direct = ns <= K.kBandDirect or (ns <= K.kBandSurv and not cells_ok)
        return ns, min(cells.size, K.kBandCells), int(direct), int(not direct and not cells_ok), \
            cells[:K.kBandCells]

    def check_route(self, W):
        ns, ncell, direct, over, cells = self.route()
        assert (W["ns"], W["ncell"], W["direct"], W["over"]) == (ns, ncell, direct, over), \
            (W["ns"], W["ncell"], W["direct"], W["over"], "expected", ns, ncell, direct, over)
        np.testing.assert_array_equal(W["cells"][:ncell], cells)

    def check_best(self, best, path):
        """``best`` is the np.argmax record of the alive entries."""
        c = self.c
        k = rank_first(self.oracle, c.idx, c.alive)
        assert k == rank_first(self.dense, c.idx, c.alive)
        assert gap_ok(self.oracle, c.y, c.alive, k) and gap_ok(self.dense, c.y, c.alive, k), \
            "the crafted y do not separate the winner: choose others"
        assert best["index"] == c.idx[k], (int(best["index"]), int(c.idx[k]), float(best["score"]),
                                           self.dense[k], self.oracle[k])
        assert best["n_scored"] == self.S.n_cand
        B.assert_value_is(best["value"], c.y[k], self.kind)
        s = float(best["score"])
        np.testing.assert_allclose(s, self.dense[k], rtol=1e-12, atol=1e-12, equal_nan=True)
        np.testing.assert_allclose(s, self.oracle[k], rtol=1e-6, atol=1e-9, equal_nan=True)
        if s == s:
            d = abs(s - self.dense[k])
            m = MAXDIFF.setdefault(path, [0.0, 0.0, 0.0])
            m[0], m[1] = max(m[0], d), max(m[1], d / max(1.0, abs(s)))
            m[2] = max(m[2], abs(s - self.oracle[k]))
        return k

    def peel(self, path, n_peel=N_PEEL):
        """Replay, check, take the winner out of the band (a spare of its cell
        in: ns and the cells stay), n_peel times; returns the winners' records."""
        c, out = self.c, []
        for _ in range(min(n_peel, int(c.alive.sum()))):
            (best,), (W,) = self.S.replay([c], j0=self.j)
            self.check_route(W)
            k = self.check_best(best, path)
            out.append((k, best))
            c.set_alive(k, False)
            if self.spare_of is not None:
                sp = [q for q in self.spare_of[k] if not c.alive[q] and q not in
                      [w for w, _ in out]]
                c.set_alive(sp[0], True)
        return out


def _indices(rng, n):
    """n distinct candidate indices past 2^33, in no order."""
    i = np.unique(rng.randint(1 << 33, 1 << 41, size=2 * n + 8, dtype=np.int64))
    assert i.size >= n
    return rng.permutation(i)[:n]


# ---------------------------------------------------------------------------
# the direct sum
# ---------------------------------------------------------------------------
def _direct_case(S, eng64, ns, rng, j=0):
    """ns survivors for the direct sum: on the grid, and from 7 on two NaN,
    survivors off the grid -- one far off (60, -60, and for GMM1 1e3, -1e3, in
    turn over the cases), one just below the grid and from 9 on one just above
    -- and the best y three times, at descending indices in entry order.
    Far from the observations both mixtures are their prior component and
    the score is one constant: of the y's drawn, those are kept whose oracle
    scores differ pairwise (by 1e-7 max(1, |s|)), the far one first."""
    kind, args = S.kinds[j]
    tab = S.tables[j]
    off = []
    if ns >= 7:
        far = (60.0, -60.0) if kind in B.LGMM else (60.0, -1e3, -60.0, 1e3)
        o, h, nb = float(tab["origin"]), float(tab["h"]), int(tab["nb"])
        off = [far[(ns + j + CONT.index((kind, args))) % len(far)], o - 3.3 * h]
        if ns >= 9:
            off.append(o + (2 * nb + 2.7) * h)
        assert np.all(band_cell(tab, off) == -2)
    n_nan = n_dup = 2 if ns >= 7 else 0
    need = ns - n_nan - n_dup
    pool = np.concatenate([np.asarray(off, np.float32),
                           y_in_cells(tab, rng.randint(int(tab["nb"]), size=4 * ns + 8), rng)])
    below, above = S.hist[j]
    sc = B.oracle_scores(kind, args, below, above, B.cand_value(pool, kind))
    keep = []
    for k in range(pool.size):
        if all(abs(sc[k] - sc[q]) > 1e-7 * max(1.0, abs(sc[k])) for q in keep):
            keep.append(k)
        if len(keep) == need:
            break
    assert len(keep) == need and (not off or keep[0] == 0)
    top = pool[keep[int(np.argmax(sc[keep]))]]
    y = np.concatenate([pool[keep], np.full(n_nan, np.nan, np.float32),
                        np.full(n_dup, top, np.float32)])
    y = y[rng.permutation(ns)].astype(np.float32)
    idx = _indices(rng, ns)
    dup = np.flatnonzero(y.view(np.uint32) == top.view(np.uint32))
    idx[dup] = np.sort(idx[dup])[::-1]
    return Case(S, eng64, Crafted(S.nt, y, idx, np.ones(ns, bool), rng), j)


def _check_direct(case, path):
    c = case.c
    wins = case.peel(path)
    # the copies of one y: in index order, the same score bits
    bits = {}
    for k, best in wins:
        bits.setdefault(c.y[k].tobytes(), []).append((int(best["index"]), best["score"].tobytes()))
    for v in bits.values():
        assert [i for i, _ in v] == sorted(i for i, _ in v)
        assert len({b for _, b in v}) == 1 or np.isnan(np.frombuffer(v[0][1], np.float64)[0])


@pytest.mark.parametrize("ns", [1, 7, 8, 9, 127, 128])
@pytest.mark.parametrize("kind,args", CONT)
def test_direct(eng64, kind, args, ns):
    """ns <= kBandDirect survivors over tiles of 0, 1, 0, 255, 3, ... entries:
    batches of kSurvBatch, survivors off the grid and NaN stay direct."""
    S = setup([(kind, args)], 2000)
    K = S.K
    assert ns <= K.kBandDirect
    rng = np.random.RandomState(ns)
    case = _direct_case(S, eng64, ns, rng)
    assert case.route()[2:4] == (1, 0)
    _check_direct(case, "direct")


@pytest.mark.parametrize("n_hist", [3, 10000])
@pytest.mark.parametrize("kind,args", CONT)
def test_direct_short_and_long_history(eng64, kind, args, n_hist):
    """3 trials: a block's component chunk holds at most one component (most
    none); 10 000: a chunk past kDirStage, the unstaged loop."""
    S = setup([(kind, args)], n_hist)
    for ns in (9, S.K.kBandDirect):
        _check_direct(_direct_case(S, eng64, ns, np.random.RandomState(n_hist + ns)),
                      "direct, %d trials" % n_hist)


# ---------------------------------------------------------------------------
# the cell expansions
# ---------------------------------------------------------------------------
def _cells_case(S, eng64, ncell, ns, rng, j=0, spares=N_PEEL, place_one_tile=False):
    """ns survivors over ncell cells (each holds one at least), and per cell
    ``spares`` entries below G that replace its peeled winners."""
    tab = S.tables[j]
    cells = pick_cells(tab, ncell, rng)
    cell = np.concatenate([cells, cells[rng.randint(ncell, size=ns - ncell)],
                           np.repeat(cells, spares)])
    alive = np.arange(cell.size) < ns
    perm = rng.permutation(cell.size)
    cell, alive = cell[perm], alive[perm]
    y = y_in_cells(tab, cell, rng)
    spare_of = {}
    for cl in cells:
        m = np.flatnonzero(cell == cl)
        sp = [int(q) for q in m if not alive[q]]
        for q in m:
            spare_of[int(q)] = sp
    return Case(S, eng64, Crafted(S.nt, y, _indices(rng, y.size), alive, rng), j,
                spare_of if spares else None)


CELLS = [(1, 129), (2, 600), (3, 600), (16, 600), (17, 600), (64, 600), (3, 4100), (3, 5000)]


@pytest.mark.parametrize("ncell,ns", CELLS)
@pytest.mark.parametrize("kind,args", CONT)
def test_cells(eng64, kind, args, ncell, ns):
    """ns > kBandDirect survivors on the grid: degree-20 expansions per listed
    cell in max(1, kBandBlocks / ncell) chunks (8, 5, 1, 1 here, and units
    past kBandBlocks), merged and evaluated by k_band_final -- 4100 and 5000:
    a second staging round of a block, and a second entry window of k_band
    whose boundary falls inside a tile."""
    S = setup([(kind, args)], 2000)
    K = S.K
    assert ns > K.kBandDirect and ncell <= K.kBandCells
    case = _cells_case(S, eng64, ncell, ns, np.random.RandomState(1000 * ncell + ns))
    assert case.route()[:4] == (ns, ncell, 0, 0)
    if ns > 4096:
        ends = np.cumsum(case.c.counts * case.c.read)
        assert case.c.n_ent > 2048 and 2048 not in ends and 4096 not in ends
    case.peel("cells")


@pytest.mark.parametrize("ncell,ns", CELLS[:3])
@pytest.mark.parametrize("kind,args", CONT)
def test_cells_small_table(eng64, kind, args, ncell, ns):
    """A cell budget of 8: wide cells, so components whose series converges
    slowly (rho > 1.5) are summed term by term or send the cell to the
    direct sum -- the same scores."""
    S = setup([(kind, args)], 2000, table_cap=8)
    assert S.stats["failed_cells"] > 0 and int(S.tables[0]["nb"]) <= 8
    case = _cells_case(S, eng64, ncell, ns, np.random.RandomState(8000 * ncell + ns))
    assert case.route()[:4] == (ns, ncell, 0, 0)
    case.peel("cells, 8-cell table")


# ---------------------------------------------------------------------------
# the exact-fallback exits
# ---------------------------------------------------------------------------
def _check_exit(S, case, rng, late, j=0):
    """The job leaves with the fp32 partials' winner and n_scored = -1."""
    want = case.c.partials(rng)
    (best,), (W,) = S.replay([case.c], j0=j)
    assert W["over"] == 1
    if late:  # (the exits after the survivors are counted leave the whole route)
        case.check_route(W)
    assert (float(best["score"]), int(best["index"]), float(best["value"]),
            int(best["n_scored"])) == want + (-1,)


@pytest.mark.parametrize("kind,args", CONT)
def test_exit_too_many_cells(eng64, kind, args):
    S = setup([(kind, args)], 2000)
    K = S.K
    rng = np.random.RandomState(65)
    case = _cells_case(S, eng64, K.kBandCells + 1, K.kBandDirect + 1, rng, spares=0)
    assert case.route()[:4] == (K.kBandDirect + 1, K.kBandCells, 0, 1)
    _check_exit(S, case, rng, True)


@pytest.mark.parametrize("kind,args", CONT)
def test_exit_survivor_off_the_grid(eng64, kind, args):
    S = setup([(kind, args)], 2000)
    K = S.K
    rng = np.random.RandomState(66)
    case = _cells_case(S, eng64, 2, K.kBandDirect + 1, rng, spares=0)
    k = int(np.flatnonzero(case.c.alive)[40])
    for y in (60.0, np.nan):
        case.c.y[k] = y
        case.c.band["y"][case.c.tile[k], case.c.slot[k]] = y
        case.cell = band_cell(S.tables[0], case.c.y)
        assert case.route()[:4] == (K.kBandDirect + 1, 2, 0, 1)
        _check_exit(S, case, rng, True)


def _one_cell(S, n, rng):
    """n survivors in one cell, no reference (the job takes an exit)."""
    y = y_in_cells(S.tables[0], np.full(n, int(S.tables[0]["nb"]) // 2), rng)
    return Crafted(S.nt, y, _indices(rng, n), np.ones(n, bool), rng)


def test_exit_too_many_survivors(eng64):
    kind, args = CONT[0]
    K = B.layout()
    ns = K.kBandSurvMax + 1
    S = setup([(kind, args)], 2000, n_tiles=-(-ns // K.kTileSlots) + 7)
    assert S.nt == 264
    rng = np.random.RandomState(67)
    c = _one_cell(S, ns, rng)
    want = c.partials(rng)
    (best,), (W,) = S.replay([c])
    assert (W["ns"], W["ncell"], W["direct"], W["over"]) == (ns, 1, 0, 1)
    assert (float(best["score"]), int(best["index"]), float(best["value"]),
            int(best["n_scored"])) == want + (-1,)
    # one survivor fewer: the cells path again, on the same (not zeroed) work
    c.set_alive(5, False)
    (best,), (W,) = S.replay([c], zero=False)
    assert (W["ns"], W["ncell"], W["direct"], W["over"]) == (K.kBandSurvMax, 1, 0, 0)
    assert best["n_scored"] == S.n_cand and best["index"] in c.idx[c.alive]


def test_exit_too_many_tiles(eng64):
    """More tiles than k_band's LDS prefix holds: the exit before any entry
    is read, whatever the tiles hold."""
    kind, args = CONT[0]
    K = B.layout()
    S = setup([(kind, args)], 2000, n_tiles=K.kBandTiles + 1)
    r, = S.res  # the level itself: re-scored exactly by the engine
    assert r.n_scored == S.n_cand and S.eng.band_overflows == 1
    rng = np.random.RandomState(68)
    c = _one_cell(S, 9, rng)
    want = c.partials(rng)
    (best,), (W,) = S.replay([c])
    assert W["over"] == 1
    assert (float(best["score"]), int(best["index"]), float(best["value"]),
            int(best["n_scored"])) == want + (-1,)
    _setups.pop(((CONT[0],), 2000, K.kBandTiles + 1, None))  # (its buffers are large)


@pytest.mark.parametrize("kind,args", CONT)
def test_full_tile_that_matters_and_not(eng64, kind, args):
    """A tile that did not fit its entries: with hi_max >= G the job exits;
    with hi_max < G it cannot hold the winner, and the job is decided."""
    S = setup([(kind, args)], 2000)
    for ns, path in ((9, "direct"), (300, "cells")):
        rng = np.random.RandomState(69 + ns)
        case = _direct_case(S, eng64, ns, rng) if ns == 9 else \
            _cells_case(S, eng64, 3, ns, rng, spares=0)
        t = int(np.flatnonzero(case.c.counts == 0)[0])
        case.c.full(t, True)
        _check_exit(S, case, rng, False)
        case.c.full(t, False)
        (best,), (W,) = S.replay([case.c], zero=False)
        case.check_route(W)
        case.check_best(best, path)


# ---------------------------------------------------------------------------
# state and sharding
# ---------------------------------------------------------------------------
def _five(S, eng64, rng, j=0):
    """A full-tile overflow, a direct job, a cells job, a job over too many
    cells: (name, case, exits)."""
    K = S.K
    over = _direct_case(S, eng64, 9, rng, j)
    over.c.full(int(np.flatnonzero(over.c.counts == 0)[0]), True)
    over.c.partials(rng)
    many = _cells_case(S, eng64, K.kBandCells + 1, 200, rng, j, spares=0)
    many.c.partials(rng)
    return [("overflow", over, True), ("direct", _direct_case(S, eng64, 100, rng, j), False),
            ("cells", _cells_case(S, eng64, 5, 700, rng, j, spares=0), False),
            ("too many cells", many, True)]


@pytest.mark.parametrize("kind,args", CONT)
def test_work_buffer_carries_no_state(eng64, kind, args):
    """The band work is zeroed only when it is allocated: an overflowed job,
    a direct one, a cells one, one over too many cells and the direct one
    again on the same buffer each give what they give on a zeroed one."""
    S = setup([(kind, args)], 2000)
    jobs = _five(S, eng64, np.random.RandomState(70))
    clean = {}
    for name, case, exits in jobs:
        (best,), (W,) = S.replay([case.c], zero=True)
        clean[name] = (best.tobytes(), {k: v for k, v in W.items() if k != "cells"})
        assert W["over"] == int(exits) and (best["n_scored"] == -1) == exits
        if not exits:
            case.check_route(W)
            case.check_best(best, name)
    S.eng._bufs["band_work"].zero_()
    for name, case, exits in jobs + [jobs[1]]:
        (best,), (W,) = S.replay([case.c], zero=False)
        assert best.tobytes() == clean[name][0], name
        assert W["over"] == clean[name][1]["over"], name
        if name != "overflow":  # (the early exit leaves the route as it was)
            assert {k: v for k, v in W.items() if k != "cells"} == clean[name][1], name


def test_three_jobs_in_one_launch(eng64):
    """A direct, a cells and an overflowed job in one launch: each job's
    result is its single-job result, bit for bit."""
    S = setup([CONT[0], CONT[1], CONT[3]], 2000)
    rng = np.random.RandomState(71)
    cases = [_direct_case(S, eng64, 100, rng, 0), _cells_case(S, eng64, 5, 700, rng, 1, spares=0),
             _direct_case(S, eng64, 9, rng, 2)]
    cases[2].c.full(int(np.flatnonzero(cases[2].c.counts == 0)[0]), True)
    cases[2].c.partials(rng)
    single = [S.replay([case.c], j0=j)[0][0] for j, case in enumerate(cases)]
    best, Ws = S.replay([case.c for case in cases])
    for j, case in enumerate(cases):
        assert best[j].tobytes() == single[j].tobytes(), j
    for j in (0, 1):
        cases[j].check_route(Ws[j])
        cases[j].check_best(best[j], ("direct", "cells")[j])
    assert Ws[2]["over"] == 1 and best[2]["n_scored"] == -1


@pytest.mark.parametrize("ns", [100, 200])
@pytest.mark.parametrize("kind,args", CONT)
def test_score_bits_do_not_depend_on_the_tiles(eng64, kind, args, ns):
    """The same survivors in one tile and spread over all 24: the same
    winners with the same score bits (a survivor's score is a function of its
    y alone, whatever the sharding of the candidates)."""
    S = setup([(kind, args)], 2000)
    K = S.K
    rng = np.random.RandomState(72 + ns)
    a = _direct_case(S, eng64, ns, rng) if ns <= K.kBandDirect else \
        _cells_case(S, eng64, 2, ns, rng, spares=0)
    n = a.c.y.size
    order = rng.permutation(n)  # another entry order as well
    one = [0] * S.nt
    one[7] = K.kTileSlots
    spread = [K.kTileSlots // 2] * S.nt
    place = np.sort(rng.choice(sum(spread), n, replace=False))
    b = Case(S, eng64, Crafted(S.nt, a.c.y[order], a.c.idx[order], a.c.alive[order], rng,
                               counts=one), 0)
    c = Case(S, eng64, Crafted(S.nt, a.c.y, a.c.idx, a.c.alive, rng, counts=spread, place=place), 0)
    path = "direct" if ns <= K.kBandDirect else "cells"
    wins = [x.peel(path, 8) for x in (a, b, c)]
    for wa, wb, wc in zip(*wins):
        assert wa[1].tobytes() == wb[1].tobytes() == wc[1].tobytes()
