"""The cell table read back cell by cell (test_gpu_table_cells.py; band_cell
is shared with test_gpu_band_paths.py): a job's tpe_table record, its region
of the engine's cell buffer decoded into exact doubles, its slices of the
plan's reach windows and wide list, the points of a cell as the kernels form
them, and the fp64 reference of what a cell stores.  The plan alone
(read_plan, check_plan) is shared with test_gpu_pruned64_stages.py: the
pruned exact fp64 scorer asks for the same plan with its own margin and draw
bound and builds no cells.
"""
import numpy as np

from hyperopt_amd import _lib as L
from oracle import tpe_oracle as O

LGMM = ("loguniform", "lognormal")
K_P, K_P32, SLOT_B, CELL_B = 9, 6, 128, 64  # tpe_table.hpp: kP, kP32, kSlotB, kCellF * 4
U_FIT = 1.0501    # |u| the table's bounds cover (kUFit)
COOP_CELLS = 4096  # kCoopCells: tables of at most this many cells build a quad per block
DRAW_Z = 5.8      # kDrawZ
RHO_LIM = 5.8     # kRhoLim
TAU_TABLE = 17.0  # TPE_TAU_TABLE
DRAW_Z64 = 8.7    # kDrawZ64 (tpe_pruned64.hip)
TAU_EXACT = 40.0  # kTauExact (tpe_pruned64.hip)
AB_MAX = 0.6768   # kAbMax


# ---------------------------------------------------------------------------
# the table's cells, as the kernels form them
# ---------------------------------------------------------------------------
def cell_centre(tab, c):
    """cell_centre (tpe_table.hpp) in numpy: the fp32 centre of cell c."""
    g0, h32 = np.float32(tab["origin"]), np.float32(tab["h"])
    c = np.asarray(c, np.int64)
    return ((2 * c + 1).astype(np.float64) * np.float64(h32) + np.float64(g0)).astype(np.float32)


def band_cell(tab, y):
    """band_cell (tpe_band.hip) in numpy: the fp32 cell of y, -2 off the grid."""
    y = np.asarray(y, np.float32)
    g0, inv_w = np.float32(tab["origin"]), np.float32(tab["inv_w"])
    nb = int(tab["nb"])
    with np.errstate(all="ignore"):
        t = (y - g0) * inv_w
        c = np.where(t >= 0, np.minimum(t, np.float32(nb)), np.float32(0)).astype(np.int64)
        c = np.minimum(c, nb - 1)
        centre = cell_centre(tab, c)
        u = (y.astype(np.float64) - centre.astype(np.float64)) / float(tab["h"])
        ok = (np.abs(u) <= np.float64(np.float32(1.05))) & (y == y)
    return np.where(ok, c, -2)


def cell_points(tab, cells, U, kind):
    """The points u of ``U`` ([cell, point] or [point]) on the cells ``cells``:
    (y = centre + h u in fp64 around the fp32 centre, the candidate value y
    or exp(y))."""
    cells = np.asarray(cells, np.int64)
    U = np.broadcast_to(np.asarray(U, np.float64), (cells.size,) + np.shape(U)[-1:])
    y = cell_centre(tab, cells).astype(np.float64)[:, None] + float(tab["h"]) * U
    return y, (np.exp(y) if kind in LGMM else y)


def ref(kind, args, below, above, value):
    """(L_below, L_above): the oracle's fp64 log-densities at ``value`` in the
    table's coordinate -- for the LGMM1 kinds the density in y = log x, i.e.
    lognormal_lpdf's -log(x) taken out again (k_score_table's outputs
    subtracts y from what the table holds)."""
    value = np.asarray(value, np.float64)
    with np.errstate(all="ignore"):
        r = O.continuous_label_scores(kind, args, below, above, value.ravel())
    bl, al = r["below_llik"].reshape(value.shape), r["above_llik"].reshape(value.shape)
    if kind in LGMM:
        y = np.log(value)
        bl, al = bl + y, al + y
    return bl, al


# ---------------------------------------------------------------------------
# a job's table, read back
# ---------------------------------------------------------------------------
class Table(object):
    """Job ``pos`` of the level an engine just ran with scorer="table".

    tab: its tpe_table record; job, seg_b, seg_a: its tpe_job and (host)
    segment records; raw: its whole region of the cell buffer (bytes);
    Pb, Pa [nb, 9]: the stored coefficients as exact doubles; off [nb]: dword
    15; m [nb, 2]: the (m_below, m_above) pairs; q [nb, 4]: the score cubics;
    coef_b / coef_a [nc, 4]: the mixtures' fp64 coefficients {mu, inv, lc, w};
    mu_b, sigma_b: the below components; reach_hi / reach_lo / wide: (below,
    above) slices of the plan's arrays."""

    @property
    def flagged(self):
        return np.isnan(self.off)

    @property
    def qflagged(self):
        return np.isnan(self.q[:, 0])

    def cell_bytes(self):
        """What the kernels wrote for cells < nb: cells, m pairs, score cells."""
        nb, cap = self.nb, self.cap
        o = (cap * 72 + 15) & ~15
        return (self.raw[:CELL_B * nb].tobytes(), self.raw[CELL_B * cap:CELL_B * cap + 8 * nb]
                .tobytes(), self.raw[o:o + 16 * nb].tobytes(), self.tab.tobytes())


def _dev(eng, name, a, b, dtype):
    return eng._bufs[name][a:b].cpu().numpy().view(dtype).copy()


def _read_plan(T, eng, pos):
    """The plan part of job ``pos``: its tpe_job, tpe_table and (host) segment
    records, and both mixtures' slices of coef64, reach_hi, reach_lo and
    wide_idx, the below mixture's of mu and sigma."""
    segs, jobs = eng.last_plan[0], eng.last_plan[3]
    T.job = job = jobs[pos].copy()
    ts = L.TABLE_DTYPE.itemsize
    T.tab = _dev(eng, "tables", ts * pos, ts * (pos + 1), L.TABLE_DTYPE)[0]
    T.seg_b, T.seg_a = segs[int(job["below"])].copy(), segs[int(job["above"])].copy()
    for half, sg in (("b", T.seg_b), ("a", T.seg_a)):
        k0, k1 = int(sg["comp_off"]), int(sg["comp_off"]) + int(sg["n_obs"]) + 1
        setattr(T, "coef_" + half, _dev(eng, "coef64", 32 * k0, 32 * k1, np.float64).reshape(-1, 4))
        setattr(T, "reach_hi_" + half, _dev(eng, "reach_hi", 8 * k0, 8 * k1, np.float64))
        setattr(T, "reach_lo_" + half, _dev(eng, "reach_lo", 8 * k0, 8 * k1, np.float64))
        setattr(T, "wide_" + half, _dev(eng, "wide_idx", 4 * k0, 4 * k1, np.int32))
        if half == "b":
            T.mu_b = _dev(eng, "mu", 8 * k0, 8 * k1, np.float64)
            T.sigma_b = _dev(eng, "sigma", 8 * k0, 8 * k1, np.float64)
    return T


def read_plan(eng, pos):
    """Job ``pos`` of the level an engine just ran with the pruned exact fp64
    scorer (precision=64, exact64="pruned"; one scorer group, so the job's
    tpe_table record is record ``pos``): the plan part of a Table -- such a
    job has no cells (tbl_cap == 0)."""
    T = _read_plan(Table(), eng, pos)
    assert int(T.job["tbl_cap"]) == 0
    T.nb = T.cap = 0
    return T


def read_table(eng, pos):
    jobs = eng.last_plan[3]
    T = _read_plan(Table(), eng, pos)
    job = T.job
    T.nb, T.cap = nb, cap = int(T.tab["nb"]), int(job["tbl_cap"])
    assert 1 <= nb <= cap
    first = int(jobs["tbl_off"][jobs["tbl_cap"] > 0].min())
    a = SLOT_B * (int(job["tbl_off"]) - first)
    T.raw = raw = _dev(eng, "cells", a, a + SLOT_B * cap, np.uint8)
    f = raw[:CELL_B * cap].view(np.float32).reshape(cap, 16)[:nb]
    t0 = 2 * 2 * K_P32  # dword 12 in halves: the fp16 pairs of n = 6..8
    tail = raw[:CELL_B * cap].view(np.float16).reshape(cap, 32)[:nb, t0:t0 + 6]
    T.Pb, T.Pa = np.empty((nb, K_P)), np.empty((nb, K_P))
    for n in range(K_P32):
        T.Pb[:, n], T.Pa[:, n] = f[:, 2 * n], f[:, 2 * n + 1]
    for n in range(K_P32, K_P):
        T.Pb[:, n], T.Pa[:, n] = tail[:, 2 * (n - K_P32)], tail[:, 2 * (n - K_P32) + 1]
    T.off = f[:, 15].astype(np.float64)
    T.m = raw[CELL_B * cap:CELL_B * cap + 8 * cap].view(np.float32).reshape(cap, 2)[:nb] \
        .astype(np.float64)
    o = (cap * 72 + 15) & ~15
    assert o + 16 * cap <= SLOT_B * cap
    T.q = raw[o:o + 16 * cap].view(np.float32).reshape(cap, 4)[:nb].astype(np.float64)
    return T


# ---------------------------------------------------------------------------
# the plan and the bound, restated
# ---------------------------------------------------------------------------
def horner(P, U):
    """sum_n P[cell, n] U[cell, point]^n in fp64."""
    out = np.zeros(U.shape)
    for n in range(P.shape[1] - 1, -1, -1):
        out = out * U + P[:, n:n + 1]
    return out


REFINE, REFINE_COMPS, REFINE_CELLS = 4, 1024, 4096  # kRefine, kRefineComps, kRefineCells


def grid_of(tab, cap, n_comp):
    """grid_of (tpe_table.hpp): (origin, h, nb) from the plan's range and
    admissible half-widths; a job of at most REFINE_COMPS components gets up
    to REFINE times the cells, never past REFINE_CELLS nor the budget."""
    lo, hi = float(tab["lo"]), float(tab["hi"])
    span = hi - lo
    hn = min(float(tab["h_below"]), float(tab["h_above"]))
    if not (hn > 0.0) or not np.isfinite(hn):
        hn = max(span, 1.0)
    if not (span > 0.0):
        return lo - hn, hn, 1
    n = np.ceil(span / (2.0 * hn))
    if n_comp <= REFINE_COMPS and n < float(REFINE_CELLS):
        n = min(n * float(REFINE), float(REFINE_CELLS))
    if not (n <= float(cap)):
        n = float(cap)
    nb = int(max(1.0, n))
    return lo, span / (2.0 * nb), nb


def plan_comp(coef, T, prior_sigma):
    """plan_comp (tpe_table.hip) for every component of a mixture: (wide,
    mu + r, mu - r, admissible half-width)."""
    mu, inv, lc = coef[:, 0], coef[:, 1], coef[:, 2]
    d = lc - T
    with np.errstate(all="ignore"):
        z = np.where(d > 0.0, np.sqrt(2.0 * np.where(d > 0.0, d, 0.0)), 0.0)
        s = (-9.0 * z + np.sqrt(81.0 * z * z + 166.0 * RHO_LIM)) / 83.0
        hk = np.where(d > 0.0, s / inv, np.inf)
        wide = inv <= 4.0 / prior_sigma  # (the prior itself: inv = 1 / prior_sigma)
        r = z / inv * (1.0 + 1e-9) + 1e-12 * np.abs(mu)
    return wide, np.where(wide, -np.inf, mu + r), np.where(wide, np.inf, mu - r), hk


def check_plan(T, reach=True):
    """The plan's windows (statement F of test_gpu_table_cells.py, whatever
    the margin and draw bound the plan was asked for): reach_hi / reach_lo are
    the running max / reversed running min of plan_comp restated from the
    record's own floors (relative 1e-12), the wide list and its counts, the
    admissible half-widths.  ``reach=False``: the reach arrays have been
    planned over since (a band overflow's exact re-score); the wide list does
    not depend on the margin."""
    tab = T.tab
    for half, seg, Tx, nwide, hx in (("b", T.seg_b, "T_below", "n_wide_below", "h_below"),
                                     ("a", T.seg_a, "T_above", "n_wide_above", "h_above")):
        coef = getattr(T, "coef_" + half)
        rh, rl = getattr(T, "reach_hi_" + half), getattr(T, "reach_lo_" + half)
        psig = float(seg["prior_sigma"])
        assert psig > 0.0 and np.all(np.diff(coef[:, 0]) >= 0.0)  # sorted by mean
        wide, hr, lr, hk = plan_comp(coef, float(tab[Tx]), psig)
        assert wide.any()  # the prior at least
        want_hi = np.maximum.accumulate(hr)
        want_lo = np.minimum.accumulate(lr[::-1])[::-1]
        for got, want in ((rh, want_hi), (rl, want_lo)) if reach else ():
            inf = np.isinf(want)
            np.testing.assert_array_equal(got[inf], want[inf])
            np.testing.assert_allclose(got[~inf], want[~inf], rtol=1e-12, atol=0)
            assert np.all(got[1:] >= got[:-1])  # non-decreasing
        # a wide component holds -inf / +inf in its own slot: the running
        # extremes pass over it unchanged
        k = np.flatnonzero(wide)
        prev = np.where(k > 0, rh[np.maximum(k - 1, 0)], -np.inf)
        nxt = np.where(k < wide.size - 1, rl[np.minimum(k + 1, wide.size - 1)], np.inf)
        if reach:
            np.testing.assert_array_equal(rh[k], prev)
            np.testing.assert_array_equal(rl[k], nxt)
        n = int(tab[nwide])
        assert n == k.size
        np.testing.assert_array_equal(getattr(T, "wide_" + half)[:n], k)
        np.testing.assert_allclose(float(tab[hx]), hk.min(), rtol=1e-12, atol=0)


def mix_eps(items, coop):
    """mix_eps (tpe_table.hip) at the admissible maximum kAbMax, as
    k_table_score stores it."""
    u, ud, ab = 2.0 ** -24, 2.0 ** -53, AB_MAX
    stride = 64 if coop else 16
    K = (items + stride - 1) // stride + 5 + (5 if coop else 0)
    E1 = np.exp(ab)
    E2 = E1 * E1
    return (4.4e-7 + np.exp(-TAU_TABLE) * 1.0001 + 0.6932 * u + 1e-13 + 2.0 ** -22
            + 5.5 * u * ab + 4.0 * u * ab * E2 + u * E2 + (K + 1) * u * 0.0198 * 1.0001
            + 1.5e-7 + 2.0 ** -25 * 4.2 * E1 + (K + 8) * 2.0 * ud * E2) * (1.0 + 1e-6)
