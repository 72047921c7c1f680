"""The cases of test_gpu_table_build_bits.py and of the script that records
its fixtures (tools/record_table_bits.py): histories, cell budgets, one build
through the engine, and a CPU restatement of how k_table_build walks a quad's
items (cell_windows, build_mix's inclusion test and per-lane scale), from
which each case's properties are asserted -- so a case cannot quietly
exercise another path than the one it is named for.

A fixture holds what the build kernels wrote for cells < nb, byte for byte:
the cell records, the (m_below, m_above) pairs, the score cells and the job's
tpe_table record (Table.cell_bytes).
"""
import os

import numpy as np

from tests import band_util as B
from tests import table_util as TU

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_bits")
N_CAND = 4096
KEY = 0x7AB1E
NO_SCALE = -100000  # kNoScale
WAVES = 4           # kBS / kWave
PARTS = ("cells", "m_pairs", "score_cells", "table")


def _gap():
    """Two tight clusters at the ends of uniform(-5, 5) and nothing between:
    the clusters' inner components have the smallest bandwidth the fit allows,
    so no window reaches the middle cells (empty windows), and the windows
    taper to nothing on the clusters' flanks (short and odd ones)."""
    rng = np.random.RandomState(8101)
    above = np.concatenate([-4.5 + 0.05 * rng.uniform(size=150), 4.4 + 0.05 * rng.uniform(size=149)])
    return "uniform", (-5.0, 5.0), rng.uniform(-5.0, 5.0, 12), rng.permutation(above)


def _late():
    """A spread history with one cluster of exact duplicates near the top of
    the range: its components carry the largest terms by far and come late in
    the sorted order, after each lane has set its scale on broad components."""
    rng = np.random.RandomState(8102)
    spread = rng.uniform(-5.0, 3.5, 300)
    c = 4.0 + 0.02 * rng.uniform(size=40)
    above = np.concatenate([spread, c, np.repeat(c[7], 200)])
    return "uniform", (-5.0, 5.0), rng.uniform(-5.0, 5.0, 30), rng.permutation(above)


def _natural(kind, args, n):
    def make():
        below, above = B.history(kind, args, n, 7300 + n)
        return kind, args, np.asarray(below, np.float64), np.asarray(above, np.float64)
    return make


# name -> (history, cell budget or None, the properties the case is there for)
CASES = {
    "coop-partial": (_natural("normal", (0.0, 2.0), 2000), 4095, ("coop", "partial")),
    "wave-partial": (_natural("normal", (0.0, 2.0), 2000), 4097, ("wave", "partial")),
    "coop-natural": (_natural("uniform", (-5.0, 5.0), 2000), None, ("coop", "wide")),
    "gap": (_gap, None, ("coop", "odd", "short", "empty", "wide")),
    "late-rescale": (_late, None, ("late", "wide")),
}


def build(eng, name):
    """The case's table, built alone through the engine and read back."""
    import hyperopt_amd.engine as E
    make, cap, _ = CASES[name]
    kind, args, below, above = make()
    work = E.LabelWork(kind, kind, args, below, above, n_cand=N_CAND, key=KEY)
    saved, over = E.TABLE_CAP, eng.band_overflows
    try:
        if cap is not None:
            E.TABLE_CAP = cap
        eng.run([work], precision=32, scorer="table")
        T = TU.read_table(eng, 0)
    finally:
        E.TABLE_CAP = saved
    # a band overflow makes the engine plan again, with the exact scorer's
    # margin, into the same reach arrays: the table's windows are gone then
    T.replanned = eng.band_overflows != over
    return T


def parts(T):
    return dict(zip(PARTS, (np.frombuffer(b, np.uint8) for b in T.cell_bytes())))


def fixture_path(name):
    return os.path.join(GOLDEN, name + ".npz")


# ---------------------------------------------------------------------------
# the walk of a quad's items, restated
# ---------------------------------------------------------------------------
def _quad_items(T, half, q):
    """(components in item order, nwin) of quad q and mixture ``half``:
    cell_windows' reach window of the quad's span, then the wide list."""
    tab, nb = T.tab, T.nb
    h = float(tab["h"])
    c0, c1 = 4 * q, min(4 * q + 3, nb - 1)
    ylo = float(TU.cell_centre(tab, c0)) - h
    yhi = float(TU.cell_centre(tab, c1)) + h
    rh, rl = getattr(T, "reach_hi_" + half), getattr(T, "reach_lo_" + half)
    lo = int(np.searchsorted(rh, ylo, side="left"))    # first k with reach_hi[k] >= ylo
    end = int(np.searchsorted(rl, yhi, side="right"))  # first k with reach_lo[k] > yhi
    nwin = max(0, end - lo)
    n_wide = int(tab["n_wide_below" if half == "b" else "n_wide_above"])
    wide = getattr(T, "wide_" + half)[:n_wide]
    return np.concatenate([np.arange(lo, lo + nwin), wide]).astype(np.int64), nwin


def _late_rescales(T, half, q, comps, nwin, coop):
    """How many lanes of quad q raise a scale they had already set: build_mix's
    walk in numpy (the inclusion test in fp32 as the kernel forms it, the
    exponent in fp64), every row and lane at once."""
    tab, nb = T.tab, T.nb
    coef, seg = getattr(T, "coef_" + half), getattr(T, "seg_" + half)
    Tf = np.float32(tab["T_below" if half == "b" else "T_above"])
    h = float(tab["h"])
    hf = np.float32(h)
    stride = 16 * WAVES if coop else 16
    cells = np.minimum(4 * q + np.arange(4), min(4 * q + 3, nb - 1))
    y0 = TU.cell_centre(tab, cells).astype(np.float64)  # [row]
    mu, inv, lc = coef[comps, 0], coef[comps, 1], coef[comps, 2]
    is_wide = (comps == int(seg["prior_pos"])) | (inv <= 4.0 / float(seg["prior_sigma"]))
    skip = (np.arange(comps.size) < nwin) & is_wide
    dy = y0[:, None] - mu[None, :]
    zn = np.maximum(np.abs(dy.astype(np.float32)) - hf, np.float32(0)) * inv.astype(np.float32)
    inc = ~skip[None, :] & (lc.astype(np.float32)[None, :] - np.float32(0.5) * zn * zn >= Tf)
    zc = dy * inv[None, :]
    t2 = (lc[None, :] - 0.5 * zc * zc) * 1.4426950408889634
    passes = (comps.size + stride - 1) // stride
    pad = passes * stride - comps.size
    inc = np.pad(inc, ((0, 0), (0, pad))).reshape(4, passes, stride)
    t2 = np.pad(t2, ((0, 0), (0, pad))).reshape(4, passes, stride)
    sl = np.full((4, stride), NO_SCALE, np.int64)
    late = np.zeros((4, stride), np.int64)
    for p in range(passes):
        up = inc[:, p] & (t2[:, p] > (sl + 8).astype(np.float64))
        late += up & (sl != NO_SCALE)
        sl = np.where(up, np.ceil(t2[:, p]).astype(np.int64), sl)
    return int(np.count_nonzero(late))


def properties(T, late_quads=64):
    """What the case's table exercises, from its plan read back.  The scale
    walk is restated on ``late_quads`` quads at a fixed stride (all of them if
    fewer)."""
    nb = T.nb
    coop = nb <= TU.COOP_CELLS
    nq = (nb + 3) // 4
    stride = 16 * WAVES if coop else 16
    P = dict(nb=nb, replanned=T.replanned, coop=coop, wave=not coop, partial=nb % 4 != 0, quads=nq,
             wide=int(T.tab["n_wide_below"]) + int(T.tab["n_wide_above"]),
             odd=0, odd_passes=0, short=0, empty=0, late=0, max_items=0)
    pick = set(np.unique(np.linspace(0, nq - 1, min(nq, late_quads)).astype(np.int64)).tolist())
    for q in range(nq):
        for half in ("b", "a"):
            comps, nwin = _quad_items(T, half, q)
            items = comps.size
            P["max_items"] = max(P["max_items"], items)
            P["odd"] += nwin % 2
            # lanes 0 .. (items - 1) % stride walk one item more than the rest
            P["odd_passes"] += ((items + stride - 1) // stride) % 2
            P["short"] += items < 16
            P["empty"] += nwin == 0
            if q in pick:
                P["late"] += _late_rescales(T, half, q, comps, nwin, coop)
    return P


def check_properties(name, P):
    """The properties the case is named for hold (at least one quad each);
    those read from the windows need the table's own plan."""
    for want in CASES[name][2]:
        assert P[want], (name, want, P)
        assert want in ("coop", "wave", "partial", "wide") or not P["replanned"], (name, want)
    # the deepest walk is the bound's summation depth, whatever the regime
    assert P["max_items"] >= 1
