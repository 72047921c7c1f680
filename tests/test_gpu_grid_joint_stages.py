"""The grid form of the joint criterion stage by stage, through the C ABI
(csrc/tpe_grid_joint.hip: tpe_grid_joint_factors, tpe_grid_joint_score; and
tpe_grid_fold_onto of csrc/tpe_grid.hip).

Expected values: tpe_joint_score on the same rows, materialised by numpy here,
under the same prepared set (tpe_joint_prep on a small synthetic history).
Every comparison is of uint64 views, exact.  T is the tile of
tpe_grid_joint_layout; the geometry cases are computed from it.
"""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import Domain, hp, rand, tpe
from hyperopt_amd import _lib as L
from hyperopt_amd import joint as J
from tests import joint_util as U

pytestmark = pytest.mark.gpu

GUARD = 8
FILL = -1234.5
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.shape(a) == np.shape(b) and (_bits(a) == _bits(b)).all()


def _layout():
    out = (ctypes.c_int64 * 4)()
    assert L.load().tpe_grid_joint_layout(ctypes.cast(out, ctypes.c_void_p), 4) == 4
    return tuple(out)


class _Problem(object):
    """A space's joint labels, a prepared set of n synthetic trials, and per
    joint label an axis of stored values (offset-free, as a pool holds them)."""

    def __init__(self, space, axes, n, seed=0, smoothing=1.0, bandwidth=0.2, lf=25,
                 prior_weight=1.0, configs=None):
        eng = tpe.engine()
        self.eng, self.t, self.lib = eng, eng.torch, eng.lib
        self.domain = Domain(lambda x: 0, space)
        labels = list(self.domain.params)
        models = J.label_models(self.domain)
        assert [m.label for m in models] == labels  # flat: every label is joint
        self.dj = J._device_labels(eng, models, smoothing)
        self.D, self.n, self.n_cols = len(models), n, len(labels)
        self.sp = ctypes.c_void_p(self.t.cuda.current_stream(eng.device).cuda_stream)
        rng = np.random.RandomState(seed)
        if configs is None:
            configs = [rand.sample_config(self.domain, rng) for _ in range(n)]
        hist = np.asarray([[float(c[lab]) for c in configs] for lab in labels], np.float64)
        hist = hist.reshape(self.n_cols, n)
        hv = self._up(hist) if n else None
        ha = self._up(np.ones((self.n_cols, max(n, 1)), np.uint8)) if n else None
        sig = J.bandwidths(models, n, bandwidth)
        some = sig > 0.0
        r = np.where(some, 1.0 / (np.sqrt(2.0) * np.where(some, sig, 1.0)), 0.0)
        head = np.concatenate([J.log_weights(n, lf, prior_weight), sig, r])
        self.dset = self.t.empty(self.lib.tpe_joint_set_doubles(self.D, n), dtype=self.t.float64,
                                 device=eng.device)
        self.dset[:head.size].copy_(self.t.from_numpy(head))
        L.check(self.lib.tpe_joint_prep(self.dj.host.ctypes.data, self.dj.dev.data_ptr(), self.D,
                                        None if hv is None else hv.data_ptr(),
                                        None if ha is None else ha.data_ptr(), n, self.n_cols,
                                        None, n, self.dset.data_ptr(), self.sp), "tpe_joint_prep")
        self.axes = [np.asarray(a, np.float64) for a in axes]
        assert len(self.axes) == self.D
        self.axis_len = np.asarray([a.size for a in self.axes], np.int64)
        self.axis_off = np.concatenate([[0], np.cumsum(self.axis_len)[:-1]]).astype(np.int64)
        self.frow0 = self.axis_off.copy()  # F rows in the axes' own order
        self.n_frows = int(self.axis_len.sum())
        self.d_axes = self._up(np.concatenate(self.axes))
        self.chunk = self.lib.tpe_joint_chunk()
        self.chunks = (n + 1 + self.chunk - 1) // self.chunk
        self.tab = None if self.dj.tables is None else self.dj.tables.data_ptr()

    def _up(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a)).to(self.eng.device)

    def factors(self, c0=0, nc=None, extra_ld=0):
        """F of the component window of chunks [c0, c0 + nc): (tensor, ldF)."""
        nc = self.chunks - c0 if nc is None else nc
        ldF = nc * self.chunk + extra_ld
        F = self.t.full((self.n_frows * ldF + GUARD,), FILL, dtype=self.t.float64,
                        device=self.eng.device)
        L.check(self.lib.tpe_grid_joint_factors(
            self.dj.host.ctypes.data, self.dj.dev.data_ptr(), self.D, self.tab, self.dj.n_tables,
            self.dset.data_ptr(), self.n, self.d_axes.data_ptr(), int(self.d_axes.numel()),
            self.axis_off.ctypes.data, self.axis_len.ctypes.data, self.frow0.ctypes.data,
            F.data_ptr(), ldF, self.n_frows, c0 * self.chunk, nc * self.chunk, self.sp),
            "tpe_grid_joint_factors")
        return F, ldF

    def whole(self):
        if not hasattr(self, "_whole"):
            self._whole = self.factors()
        return self._whole

    def grid(self, block, row_begin, n_rows, windows=None, sub=None, prefill=FILL,
             mode=L.GRID_JOINT_STORE, pad=GUARD):
        """tpe_grid_joint_score over ``block`` = [(radix, joint label or None,
        pos)]: out[pad:pad + n_rows], its guards checked.  ``windows``: [(c0,
        nc)] component windows, each with an F of its own (None: one, whole)."""
        t = self.t
        radix = np.asarray([b[0] for b in block], np.int64)
        frow = np.asarray([-1 if b[1] is None else self.frow0[b[1]] + b[2] for b in block],
                          np.int64)
        assert [b[1] for b in block if b[1] is not None] == list(range(self.D))
        out = t.full((n_rows + 2 * pad,), prefill, dtype=t.float64, device=self.eng.device)
        need = self.lib.tpe_grid_joint_scratch_bytes(n_rows, self.n)
        assert need == 16 * n_rows * self.chunks
        scratch = t.full((need + 64,), 0xA5, dtype=t.uint8, device=self.eng.device)
        tables = [(self.whole(), 0, self.chunks)] if windows is None else \
            [(self.factors(c0, nc, extra_ld=2 * k), c0, nc) for k, (c0, nc) in enumerate(windows)]
        for (F, ldF), c0, nc in tables:
            L.check(self.lib.tpe_grid_joint_score(
                F.data_ptr(), ldF, self.n_frows, c0 * self.chunk, nc * self.chunk,
                self.dset.data_ptr(), self.n, radix.ctypes.data, frow.ctypes.data, len(block),
                row_begin, n_rows, None if sub is None else sub.data_ptr(),
                out.data_ptr() + 8 * pad, mode, scratch.data_ptr(),
                1 if c0 + nc >= self.chunks else 0, self.sp), "tpe_grid_joint_score")
        t.cuda.synchronize()
        for (F, ldF), _c0, _nc in tables:
            assert (F[self.n_frows * ldF:].cpu().numpy() == FILL).all()
        o = out.cpu().numpy()
        assert _same_bits(o[:pad], np.full(pad, prefill))
        assert _same_bits(o[pad + n_rows:], np.full(pad, prefill))
        assert (scratch[need:].cpu().numpy() == 0xA5).all()
        return o[pad:pad + n_rows]

    def rows(self, block, row_begin, n_rows):
        """The rows' values, label-major (n_cols, n_rows), by numpy."""
        idx = np.arange(row_begin, row_begin + n_rows, dtype=np.int64)
        vals = np.full((self.n_cols, n_rows), np.nan)
        for radix, d, pos in reversed(block):
            idx, digit = np.divmod(idx, radix)
            if d is not None:
                vals[self.dj.host["col"][d]] = self.axes[d][pos + digit]
        assert (idx == 0).all()
        return vals

    def dense(self, block, row_begin, n_rows, sub=None):
        """tpe_joint_score on the materialised rows."""
        t = self.t
        vals = self._up(self.rows(block, row_begin, n_rows))
        out = t.full((n_rows,), FILL, dtype=t.float64, device=self.eng.device)
        scratch = t.empty(max(self.lib.tpe_joint_scratch_bytes(n_rows, self.n), 16),
                          dtype=t.uint8, device=self.eng.device)
        L.check(self.lib.tpe_joint_score(
            self.dj.host.ctypes.data, self.dj.dev.data_ptr(), self.D, self.tab, self.dj.n_tables,
            self.dset.data_ptr(), self.n, vals.data_ptr(), n_rows, self.n_cols, 0, n_rows,
            None if sub is None else sub.data_ptr(), out.data_ptr(), scratch.data_ptr(), self.sp),
            "tpe_joint_score")
        return out.cpu().numpy()


# -- the geometry space: D labels of three kinds, axes of any length -----------------
def _geo_space(D):
    kinds = [lambda s: hp.uniform(s, 0, 1), lambda s: hp.quniform(s, 0, 1000, 1),
             lambda s: hp.normal(s, 0, 1)]
    return [kinds[i % 3]("l%02d" % i) for i in range(D)]


def _geo_axes(lengths, seed=1):
    rng = np.random.RandomState(seed)
    out = []
    for i, m in enumerate(lengths):
        out.append([rng.uniform(size=m), rng.permutation(1001)[:m].astype(np.float64),
                    rng.normal(size=m)][i % 3])
    return out


def _geo(name, radices, n=19):
    """A block whose labels are all joint, label i of radix radices[i] with an
    axis two values longer (pos = 1: neither end of the axis is digit 0)."""
    key = (name, tuple(radices), n)
    if key not in _CACHE:
        p = _Problem(_geo_space(len(radices)), _geo_axes([r + 2 for r in radices]), n)
        _CACHE[key] = (p, [(r, d, 1) for d, r in enumerate(radices)])
    return _CACHE[key]


def _windows(T, total):
    """(row_begin, n_rows): the issue's row counts at its row_begins, clipped."""
    out = []
    for r0 in (0, 1, T - 1, total // 2 + 3):
        for k in (1, T - 1, T, T + 1, 2 * T + 5):
            if r0 + k <= total:
                out.append((r0, k))
    return out


def _check_block(p, block, windows):
    for r0, k in windows:
        got, want = p.grid(block, r0, k), p.dense(block, r0, k)
        assert _same_bits(got, want), (r0, k, np.flatnonzero(_bits(got) != _bits(want))[:8])
        assert np.isfinite(want).all()


def test_many_fast_labels():
    T = _layout()[0]
    radices = [2, 3, 2, 5, 2, 2, 3, 2, 2, 3, 2, 2]
    p, block = _geo("small", radices)
    total = int(np.prod(radices))
    assert total > 4 * T
    _check_block(p, block, _windows(T, total) + [(total - T - 7, T + 7)])


def test_a_last_label_wider_than_the_tile():
    T = _layout()[0]
    radices = [2, 3, 2, T + 44]
    p, block = _geo("wide_last", radices)
    total = int(np.prod(radices))
    _check_block(p, block, _windows(T, total) + [(0, total)])


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_a_stride_next_to_the_tile(delta):
    T = _layout()[0]
    radices = [3, 4, T + delta]  # label 1 has stride T - 1, T, T + 1
    p, block = _geo("stride%d" % delta, radices)
    total = int(np.prod(radices))
    _check_block(p, block, _windows(T, total) + [(0, total)])


def test_radix_one_labels_and_a_label_that_only_decodes():
    T = _layout()[0]
    radices = [1, 3, 1, 5, 7, 1, 4, 1]  # radix 1 first, in the middle, last
    p, block = _geo("ones", radices)
    total = int(np.prod(radices))
    _check_block(p, block, [(0, total), (1, T), (T - 1, total - T + 1), (17, 2)])
    # decode-only labels (frow = -1) between joint ones, of radix 6, 1 and 2
    mixed = block[:2] + [(6, None, 0)] + block[2:5] + [(1, None, 0), (2, None, 0)] + block[5:]
    assert int(np.prod([b[0] for b in mixed])) == 12 * total
    _check_block(p, mixed, _windows(T, 12 * total))
    # ... and first and last
    ends = [(5, None, 0)] + block + [(3, None, 0)]
    _check_block(p, ends, [(0, 15 * total), (T + 1, 2 * T + 5)])


def test_one_joint_label_and_a_block_of_one_row():
    T = _layout()[0]
    p, block = _geo("single", [2 * T + 9])
    _check_block(p, block, _windows(T, 2 * T + 9) + [(0, 2 * T + 9)])
    _check_block(p, [(1, 0, 5)], [(0, 1)])          # a block of one row
    _check_block(p, [(4, None, 0), (1, 0, 0), (2, None, 0)], [(0, 8), (3, 1)])
    q, block = _geo("one_row", [1, 1, 1, 1])
    _check_block(q, block, [(0, 1)])


# -- components ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 6, 7, 8, 255, 256, 257, 513])
def test_component_counts(n):
    """The prior alone; the prior at every place of a pass; C = 0 and 1 mod the
    chunk; one, two and three chunks.  Past one chunk: F built whole, and in
    windows split at components 256 and 512, with the same bits."""
    T, chunk = _layout()[:2]
    radices = [3, 2, 5, 2, 7]
    p, block = _geo("comp", radices, n=n)
    total = int(np.prod(radices))
    want = p.dense(block, 0, total)
    got = p.grid(block, 0, total)
    assert _same_bits(got, want) and np.isfinite(want).all()
    if p.chunks == 1:
        return
    assert chunk == 256
    cuts = [(0, 1), (1, 1), (2, 1)][:p.chunks] if p.chunks == 3 else [(0, 1), (1, 1)]
    assert _same_bits(p.grid(block, 0, total, windows=cuts), want)
    Fw, ldw = p.whole()
    whole = Fw[:p.n_frows * ldw].cpu().numpy().reshape(p.n_frows, ldw)
    for c0, nc in cuts + ([(1, 2)] if p.chunks == 3 else []):
        F, ld = p.factors(c0, nc)
        part = F[:p.n_frows * ld].cpu().numpy().reshape(p.n_frows, ld)
        assert _same_bits(part, whole[:, c0 * chunk:(c0 + nc) * chunk])
    if p.chunks == 3:
        assert _same_bits(p.grid(block, 0, total, windows=[(0, 1), (1, 2)]), want)
        assert _same_bits(p.grid(block, 0, total, windows=[(0, 2), (2, 1)]), want)
    # F past the last component is padding (0.0), whatever the window
    C = n + 1
    assert (whole[:, C:] == 0.0).all() and not (whole[:, :C] == 0.0).all()


# -- kinds -------------------------------------------------------------------------------
ALL_KINDS_AXES = {
    "a": [2, 0, 1], "b": [9, 0, 4], "bb": [0, 12, 5],          # (offset-free: 12 .. 24 stored)
    "c": [4.0, 6.5, 7.0], "d": [float(np.exp(-2.0)), 0.5, 1.0],
    "e": [0.0, 9.0, 30.0],                                      # 30: no mass inside [0, 10]
    "f": [0.0, 2.0, 20.0, 400.0],                               # 0: a lower edge below 0, clipped
    "g": [-3.0, 4.0, 25.0], "h": [1e-13, 0.1, 5.0],
    "i": [-2.0, 8.0, 4000.0],                                   # 4000: mass 0 under every component
    "j": [0.0, 3.0, 1.0],                                       # 0: Phi(lower edge) = 0
    "k": [1, 2, 0],                                             # 0: prior probability 0
}


@pytest.mark.parametrize("n", [0, 40, 300])
def test_all_kinds(n):
    space = U.all_kinds_space(hp)
    labels = sorted(space)
    p = _Problem(space, [ALL_KINDS_AXES[lab] for lab in labels], n, seed=4)
    assert list(p.domain.params) == labels
    block = [(len(ALL_KINDS_AXES[lab]), d, 0) for d, lab in enumerate(labels)]
    total = int(np.prod([b[0] for b in block]))
    T = _layout()[0]
    for r0, k in [(0, 2 * T + 5), (total - T - 1, T + 1), (total // 2, T)]:
        got, want = p.grid(block, r0, k), p.dense(block, r0, k)
        assert _same_bits(got, want), (r0, k)
    # every row of a window that fixes e = 30, i = 4000 or k = 0 is -inf
    sub = [(r, d, 0) if lab not in ("e", "i", "k") else (1, d, 2)
           for d, (lab, (r, _d, _p)) in enumerate(zip(labels, block))]
    k = int(np.prod([b[0] for b in sub]))
    got, want = p.grid(sub, 0, min(k, 3 * T)), p.dense(sub, 0, min(k, 3 * T))
    assert _same_bits(got, want) and np.isneginf(want).all()
    # the factor table itself: -inf where the mass is none, no NaN among the components
    F, ld = p.whole()
    tab = F[:p.n_frows * ld].cpu().numpy().reshape(p.n_frows, ld)[:, :n + 1]
    assert not np.isnan(tab).any()
    e_row = int(p.frow0[labels.index("e")]) + 2
    assert np.isneginf(tab[e_row]).all() and np.isfinite(tab[e_row - 1]).all()


def test_zero_coordinates_and_the_ragged_pass():
    """Fit coordinates of exactly 0 next to the zero pad of a ragged last pass."""
    space = U.zero_coordinate_space(hp)
    labels = sorted(space)
    rows = U.zero_coordinate_rows()
    axes = []
    for lab in labels:  # the rows' values per label, and -0.0 next to 0.0
        axes.append(list(dict.fromkeys(float(r[lab]) for r in rows)) +
                    ([-0.0] if lab == "n" else []))
    for n in (3, 10):  # C = 4 and 11: ragged passes
        p = _Problem(space, axes, n, seed=2)
        block = [(len(a), d, 0) for d, a in enumerate(axes)]
        total = int(np.prod([b[0] for b in block]))
        got, want = p.grid(block, 0, total), p.dense(block, 0, total)
        assert _same_bits(got, want) and not np.isnan(want).any()


# -- out modes -----------------------------------------------------------------------------
def test_out_modes():
    T = _layout()[0]
    p, block = _geo("small", [2, 3, 2, 5, 2, 2, 3, 2, 2, 3, 2, 2])
    r0, k = T + 3, 2 * T + 5
    plain = p.dense(block, r0, k)
    rng = np.random.RandomState(9)
    sub_h = rng.normal(size=k)
    sub_h[5], sub_h[6] = -np.inf, np.inf
    sub = p._up(sub_h)
    with_sub = p.grid(block, r0, k, sub=sub)
    assert _same_bits(with_sub, p.dense(block, r0, k, sub=sub))
    with np.errstate(invalid="ignore"):
        assert _same_bits(with_sub, plain - sub_h)
    assert _same_bits(p.grid(block, r0, k), plain)
    # add onto a prefilled out (the guards hold the prefill too: untouched)
    for prefill in (0.0, 2.5, -1e300):
        added = p.grid(block, r0, k, sub=sub, prefill=prefill, mode=L.GRID_JOINT_ADD)
        with np.errstate(invalid="ignore"):
            assert _same_bits(added, prefill + (plain - sub_h))
    assert _same_bits(p.grid(block, r0, k, prefill=1.0, mode=L.GRID_JOINT_ADD), 1.0 + plain)
    # a sentinel fill around a window inside a longer vector
    assert _same_bits(p.grid(block, r0, k, prefill=np.nan, pad=3 * T), plain)


# -- tpe_grid_fold_onto ----------------------------------------------------------------------
FOLD_RADICES = [[4, 1, 5], [2, 3, 2, 5, 2, 2, 3], [3, 2300], [2100, 3], [1, 1, 7, 1], [2049, 2],
                [5, 2047, 1, 3]]


def _fold_numpy(bl, al, off, radix, r0, k, start):
    idx = np.arange(r0, r0 + k, dtype=np.int64)
    digits = []
    for r in reversed(radix):
        idx, dg = np.divmod(idx, r)
        digits.append(dg)
    digits.reverse()
    s = np.array(start, np.float64).copy()
    for o, dg in zip(off, digits):
        if o >= 0:
            with np.errstate(invalid="ignore"):
                s = s + (bl[o + dg] - al[o + dg])
    return s


@pytest.mark.parametrize("radix", FOLD_RADICES, ids=lambda r: "x".join(map(str, r)))
def test_fold_onto(radix):
    eng = tpe.engine()
    t, lib = eng.torch, eng.lib
    sp = ctypes.c_void_p(t.cuda.current_stream(eng.device).cuda_stream)
    rng = np.random.RandomState(len(radix))
    total = int(np.prod(radix))
    n_terms = int(sum(radix))
    bl, al = rng.normal(size=n_terms) * 3, rng.normal(size=n_terms)
    d_bl, d_al = (t.from_numpy(a).to(eng.device) for a in (bl, al))
    base = np.concatenate([[0], np.cumsum(radix)[:-1]]).astype(np.int64)
    rad = np.asarray(radix, np.int64)

    def onto(off, r0, k, start):
        S = t.full((k + 2 * GUARD,), FILL, dtype=t.float64, device=eng.device)
        S[GUARD:GUARD + k].copy_(t.from_numpy(np.ascontiguousarray(start)))
        off = np.ascontiguousarray(off, np.int64)
        L.check(lib.tpe_grid_fold_onto(d_bl.data_ptr(), d_al.data_ptr(), off.ctypes.data,
                                       rad.ctypes.data, len(radix), r0, k,
                                       S.data_ptr() + 8 * GUARD, sp), "tpe_grid_fold_onto")
        o = S.cpu().numpy()
        assert (o[:GUARD] == FILL).all() and (o[GUARD + k:] == FILL).all()
        return o[GUARD:GUARD + k]

    windows = [(0, total)] + [(r0, k) for r0, k in ((1, 2047), (2047, 2050), (total - 1, 1))
                              if r0 + k <= total]
    for r0, k in windows:
        start = rng.normal(size=k)
        assert _same_bits(onto(base, r0, k, start), _fold_numpy(bl, al, base, radix, r0, k, start))
        # from 0.0 and with every label adding: the bits of tpe_grid_fold
        S0 = t.full((k,), FILL, dtype=t.float64, device=eng.device)
        L.check(lib.tpe_grid_fold(d_bl.data_ptr(), d_al.data_ptr(), base.ctypes.data,
                                  rad.ctypes.data, len(radix), r0, k, S0.data_ptr(), sp),
                "tpe_grid_fold")
        assert _same_bits(onto(base, r0, k, np.zeros(k)), S0.cpu().numpy())
        # labels that only decode: each in turn, then every other one, then all
        skips = [[i] for i in range(len(radix))] + [list(range(0, len(radix), 2)),
                                                    list(range(len(radix)))]
        for skip in skips:
            off = base.copy()
            off[skip] = -1
            assert _same_bits(onto(off, r0, k, start),
                              _fold_numpy(bl, al, off, radix, r0, k, start)), (r0, k, skip)
