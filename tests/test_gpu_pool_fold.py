"""tpe_pool_fold alone (csrc/tpe_pool.hip), through the C ABI on synthetic
log-densities, against the sequential numpy fold: what score_configs never
hands it -- columns that are a permutation and not the identity, regions with
gaps between them, terms_ld != ld, activity bytes other than 0 and 1, noise
and live flags in the padding, inactive entries that are not finite, label
counts on both sides of the 16 labels one launch takes, init = 0.

"The same bits" as in test_gpu_grid_pool.py: NaN in the same rows (an
operation's NaN carries the sign the processor chooses), every other row bit
for bit.
"""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _lib as L
from tests.test_gpu_grid_pool import _same_bits

pytestmark = pytest.mark.gpu

POISON = -7.0
LIVE_BYTES = np.array([0, 0, 1, 2, 255], np.uint8)   # any byte but 0 is live


class Fold(object):
    """One synthetic problem: bl / al with one region per label (shuffled,
    gaps of noise between them), activity (n_cols, ld) and terms (n_cols,
    terms_ld) with more columns than labels."""

    def __init__(self, n_rows, n_labels, seed):
        import torch
        self.t, self.lib = torch, L.load()
        self.dev = torch.device("cuda", torch.cuda.current_device())
        rng = np.random.RandomState(seed)
        self.n, self.nl = n_rows, n_labels
        self.ld, self.terms_ld = n_rows + 37, n_rows + 5
        self.n_cols = n_labels + 3
        col = rng.permutation(self.n_cols)[:n_labels]
        while n_labels and np.array_equal(col, np.arange(n_labels)):
            col = rng.permutation(self.n_cols)[:n_labels]
        self.col = col.astype(np.int64)
        off, size = np.zeros(n_labels, np.int64), 3
        for i in rng.permutation(n_labels):
            off[i] = size
            size += n_rows + int(rng.randint(1, 10))
        self.off = off
        self.bl, self.al = rng.normal(size=size) * 3.0, rng.normal(size=size) * 3.0
        self.active = LIVE_BYTES[rng.randint(0, LIVE_BYTES.size, (self.n_cols, self.ld))]

    def region(self, i):
        return slice(int(self.off[i]), int(self.off[i]) + self.n)

    def on(self, i):
        return self.active[self.col[i], :self.n] != 0

    def set(self, i, row, bl, al, live):
        self.bl[self.off[i] + row], self.al[self.off[i] + row] = bl, al
        self.active[self.col[i], row] = live

    def want(self, first=0, last=None, start=None):
        """The sequential fold of labels [first, last), from 0.0 or ``start``."""
        s = np.zeros(self.n) if start is None else np.array(start, np.float64)
        with np.errstate(invalid="ignore"):
            for i in range(first, self.nl if last is None else last):
                term = self.bl[self.region(i)] - self.al[self.region(i)]
                s = np.where(self.on(i), s + term, s)
        return s

    def want_terms(self, first=0, last=None, before=None):
        out = np.full((self.n_cols, self.terms_ld), POISON) if before is None else before.copy()
        with np.errstate(invalid="ignore"):
            for i in range(first, self.nl if last is None else last):
                term = self.bl[self.region(i)] - self.al[self.region(i)]
                out[self.col[i], :self.n] = np.where(self.on(i), term, np.nan)
        return out

    def upload(self):
        t = self.t
        self.d_bl = t.from_numpy(self.bl).to(self.dev)
        self.d_al = t.from_numpy(self.al).to(self.dev)
        self.d_active = t.from_numpy(np.ascontiguousarray(self.active)).to(self.dev)
        return self

    def __call__(self, S, terms, init, first=0, last=None):
        """Labels [first, last) into the device tensors S / terms (or None)."""
        t = self.t
        last = self.nl if last is None else last
        off = np.ascontiguousarray(self.off[first:last])
        col = np.ascontiguousarray(self.col[first:last])
        sp = ctypes.c_void_p(t.cuda.current_stream(self.dev).cuda_stream)
        L.check(self.lib.tpe_pool_fold(self.d_bl.data_ptr(), self.d_al.data_ptr(), off.ctypes.data,
                                       col.ctypes.data, last - first, self.d_active.data_ptr(),
                                       self.ld, self.n, init, S.data_ptr(),
                                       None if terms is None else terms.data_ptr(),
                                       self.terms_ld, sp), "tpe_pool_fold")
        t.cuda.synchronize(self.dev)

    def new_S(self, start=None):
        S = self.t.full((self.ld,), POISON, dtype=self.t.float64, device=self.dev)
        if start is not None:
            S[:self.n].copy_(self.t.from_numpy(np.ascontiguousarray(start)))
        return S

    def new_terms(self):
        return self.t.full((self.n_cols, self.terms_ld), POISON, dtype=self.t.float64,
                           device=self.dev)

    def check(self, S, want, terms=None, want_terms=None):
        S = S.cpu().numpy()
        assert _same_bits(S[:self.n], want)
        assert (S[self.n:] == POISON).all()          # the padding of S is not written
        if terms is not None:
            # (the padding and the columns of no label keep their poison)
            assert _same_bits(terms.cpu().numpy(), want_terms)


def _plant(f):
    """Non-finite entries, where the problem has the rows and labels for them.
    Returns {row: the S it must have, as 'finite' or 'nan'}."""
    rows = {}
    if f.nl >= 2 and f.n >= 255:
        inf, nan = np.inf, np.nan
        for i in range(f.nl):      # every other label of these rows: finite and live
            for row in range(10, 17):
                f.active[f.col[i], row] = 1
        f.set(0, 10, inf, inf, 0)      # inactive inf - inf
        f.set(0, 11, nan, 1.0, 0)      # inactive nan
        f.set(0, 12, inf, 1.0, 0)      # inactive inf
        f.set(f.nl - 1, 13, -inf, -inf, 0)  # ... in the last label (the last launch)
        rows.update({10: "finite", 11: "finite", 12: "finite", 13: "finite"})
        f.set(0, 14, inf, inf, 2)      # active inf - inf
        f.set(0, 15, inf, 1.0, 255)    # +inf then -inf, two labels
        f.set(1, 15, -inf, 1.0, 1)
        rows.update({14: "nan", 15: "nan"})
        if f.nl >= 17:                 # ... and across two launches
            f.set(15, 16, inf, 1.0, 1)
            f.set(16, 16, 1.0, inf, 1)
            rows[16] = "nan"
    return rows


@pytest.mark.parametrize("n_labels", [0, 1, 16, 17, 33])
@pytest.mark.parametrize("n_rows", [1, 255, 256, 257])
def test_fold(n_rows, n_labels):
    f = Fold(n_rows, n_labels, 100 * n_rows + n_labels)
    planted = _plant(f)
    f.upload()
    if n_labels:
        assert not np.array_equal(f.col, np.arange(n_labels)) and f.terms_ld != f.ld
        assert n_labels == 1 or np.diff(np.sort(f.off)).min() > n_rows   # gaps between regions
        assert f.active[:, n_rows:].any() and {2, 255} <= set(np.unique(f.active).tolist())
    # init = 1, with terms
    want = f.want()
    S, terms = f.new_S(), f.new_terms()
    f(S, terms, 1)
    f.check(S, want, terms, f.want_terms())
    got = S.cpu().numpy()
    for row, kind in planted.items():
        assert np.isfinite(got[row]) if kind == "finite" else np.isnan(got[row]), (row, kind)
    if n_labels == 0:
        assert (got[:n_rows] == 0.0).all() and not np.signbit(got[:n_rows]).any()
    # terms = NULL: the same S
    S2 = f.new_S()
    f(S2, None, 1)
    f.check(S2, want)
    assert _same_bits(S2.cpu().numpy()[:n_rows], got[:n_rows])
    # init = 0: S continues from its content (with no label: stays as it was)
    start = np.random.RandomState(n_rows).normal(size=n_rows)
    start[0] = -0.0
    S3, terms3 = f.new_S(start), f.new_terms()
    f(S3, terms3, 0)
    f.check(S3, f.want(start=start), terms3, f.want_terms())
    if n_labels == 0:
        assert np.array_equal(S3.cpu().numpy()[:n_rows].view(np.int64), start.view(np.int64))


@pytest.mark.parametrize("cut", [5, 16])
def test_fold_in_two_calls(cut):
    """33 labels in one call, and as init = 1 with ``cut`` labels then init =
    0 with the rest: the same bits, S and terms."""
    f = Fold(257, 33, 9)
    planted = _plant(f)
    f.upload()
    S, terms = f.new_S(), f.new_terms()
    f(S, terms, 1)
    f.check(S, f.want(), terms, f.want_terms())
    S2, terms2 = f.new_S(), f.new_terms()
    f(S2, terms2, 1, 0, cut)
    half = f.want(0, cut)
    f.check(S2, half, terms2, f.want_terms(0, cut))
    f(S2, terms2, 0, cut, 33)
    f.check(S2, f.want(cut, 33, start=half), terms2, f.want_terms())
    assert _same_bits(S2.cpu().numpy(), S.cpu().numpy())
    assert _same_bits(terms2.cpu().numpy(), terms.cpu().numpy())
    got = S.cpu().numpy()
    assert planted[16] == "nan" and np.isnan(got[[14, 15, 16]]).all()
    assert np.isfinite(got[[10, 11, 12, 13]]).all()
