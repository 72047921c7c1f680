"""The kernels of ``joint="tree"`` stage by stage, through the C ABI
(csrc/tpe_joint_tree.hip): tpe_rows_compact against ``np.flatnonzero``, and
tpe_joint_score_rows against tpe_joint_score of the same rows under the same
prepared set.  Everything here is exact: rows, counts, bits, and what a call
must leave untouched (sentinel-filled buffers).
"""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _lib as L
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from hyperopt_amd import tpe

pytestmark = pytest.mark.gpu

ROW_FILL = -7            # what out_rows / the count hold before a call
FILL = -1234.5           # what an output holds before a call
GUARD = 8
_S = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.shape(a) == np.shape(b) and (_bits(a) == _bits(b)).all()


def _torch():
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    return torch, dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _up(a):
    t, dev, _ = _torch()
    return t.from_numpy(np.ascontiguousarray(a)).to(dev)


# -- 1. compact ------------------------------------------------------------------
def _layout():
    out = (ctypes.c_int64 * 2)()
    assert L.load().tpe_rows_compact_layout(ctypes.cast(out, ctypes.c_void_p), 2) == 2
    return int(out[0]), int(out[1])


def _compact(flags):
    t, dev, sp = _torch()
    lib = L.load()
    n = int(flags.size)
    need = lib.tpe_rows_compact_scratch_bytes(n)
    assert need >= 8
    d_flags = _up(np.concatenate([flags, np.full(GUARD, 0xFF, np.uint8)]))  # (set bytes past n)
    rows = t.full((n + GUARD,), ROW_FILL, dtype=t.int64, device=dev)
    count = t.full((1 + GUARD,), ROW_FILL, dtype=t.int64, device=dev)
    scratch = t.full((need + 64,), 0xA5, dtype=t.uint8, device=dev)
    L.check(lib.tpe_rows_compact(d_flags.data_ptr(), n, rows.data_ptr(), count.data_ptr(),
                                 scratch.data_ptr(), sp), "tpe_rows_compact")
    t.cuda.synchronize()
    assert (scratch[need:].cpu().numpy() == 0xA5).all()
    count = count.cpu().numpy()
    assert (count[1:] == ROW_FILL).all()
    return rows.cpu().numpy(), int(count[0])


def _patterns(n):
    rng = np.random.RandomState(n % 9973)
    out = {"zero": np.zeros(n, np.uint8), "nonzero": np.full(n, 1, np.uint8),
           "alternating": (np.arange(n) % 2).astype(np.uint8),
           "bytes": rng.choice(np.asarray([0, 0, 2, 0x80, 0xFF, 1], np.uint8), n)}
    if n:
        first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        first[0], last[-1] = 1, 0x40
        out.update(first=first, last=last)
    return out


def _compact_sizes():
    per_block, per_pass = _layout()
    assert per_block >= 256 and per_pass % per_block == 0
    return [0, 1, 255, 256, 257, per_block, per_block + 1, per_pass + 1]


@pytest.mark.parametrize("which", range(8))
def test_compact_equals_flatnonzero(which):
    """n_rows 0, 1, 255, 256, 257, one block, one more than a block handles,
    one more than one pass of the scan covers; every flag pattern."""
    n = _compact_sizes()[which]
    for name, flags in _patterns(n).items():
        rows, count = _compact(flags)
        want = np.flatnonzero(flags)
        assert count == want.size, (n, name)
        np.testing.assert_array_equal(rows[:count], want)
        assert (rows[count:] == ROW_FILL).all(), (n, name)   # nothing past the count


def test_compact_refuses_bad_arguments():
    t, dev, sp = _torch()
    lib = L.load()
    buf = t.full((64,), ROW_FILL, dtype=t.int64, device=dev)
    flags = t.ones(64, dtype=t.uint8, device=dev)
    p = buf.data_ptr()
    assert lib.tpe_rows_compact(flags.data_ptr(), -1, p, p, p, sp) == -1
    assert lib.tpe_rows_compact(flags.data_ptr(), 8, p, None, p, sp) == -1
    assert lib.tpe_rows_compact(flags.data_ptr(), 8, p, p, None, sp) == -1
    assert lib.tpe_rows_compact(None, 8, p, p, p, sp) == -1
    assert lib.tpe_rows_compact(flags.data_ptr(), 8, None, p + 8, p, sp) == -1
    assert lib.tpe_rows_compact_scratch_bytes(-1) == -1
    assert b"tpe_rows_compact" in lib.tpe_last_error()
    t.cuda.synchronize()
    assert (buf.cpu().numpy() == ROW_FILL).all()             # nothing was launched


# -- 2. score by list --------------------------------------------------------------
class _Scorer(object):
    """The all-kinds case of tests/test_gpu_joint.py on the device: 300 rows,
    a below set of 7 + 1 and an above set of 613 + 1 components, and log L of
    every row under each from tpe_joint_score."""

    def __init__(self):
        from tests.test_gpu_joint import KW, P_ROWS, _all_kinds
        t, dev, sp = _torch()
        self.lib = L.load()
        domain, trials, pool, _ = _all_kinds()
        eng = tpe.engine()
        hist = tpe.collect_history(trials, pool.labels)
        self.n_cols = len(pool.labels)
        fit, = J.fit(eng, domain, hist, pool_mod._seen_rows(eng, hist), KW["gamma"], self.n_cols,
                     KW["prior_weight"], KW["linear_forgetting"], KW["bandwidth"],
                     KW["cat_smoothing"])
        self.dj, self.sets, self.sp = fit.dj, fit.sets, fit.sp
        assert [n for _, n, _ in self.sets] == [7, 613]
        self.P = P_ROWS
        self.vals = pool.device(eng).vals
        self.ld = int(self.vals.shape[1])
        assert self.ld >= self.P
        self.n_max = 613
        self.scratch = t.empty(self.lib.tpe_joint_scratch_bytes(self.ld, self.n_max) + 64,
                               dtype=t.uint8, device=dev)
        self.dense = [self._dense(s) for s in (0, 1)]
        assert np.isneginf(self.dense[0][[5, 299]]).all()    # (the case's -inf rows are here)

    def _head(self, s):
        dj = self.dj
        dset, n, _ = self.sets[s]
        tab = None if dj.tables is None else dj.tables.data_ptr()
        return (dj.host.ctypes.data, dj.dev.data_ptr(), len(dj.models), tab, dj.n_tables,
                dset.data_ptr(), n, self.vals.data_ptr(), self.ld, self.n_cols)

    def _dense(self, s):
        t, dev, _ = _torch()
        out = t.full((self.P,), FILL, dtype=t.float64, device=dev)
        L.check(self.lib.tpe_joint_score(*self._head(s), 0, self.P, None, out.data_ptr(),
                                         self.scratch.data_ptr(), self.sp), "tpe_joint_score")
        return out.cpu().numpy()

    def call(self, s, rows, count, list_begin, max_rows, mode, out, sub=None, expect=0):
        """One tpe_joint_score_rows call; ``out``: the output's initial
        contents (numpy).  Returns what it holds afterwards."""
        t, dev, _ = _torch()
        need = self.lib.tpe_joint_scratch_bytes(max_rows, self.sets[s][1])
        self.scratch[need:].fill_(0xA5)
        d_rows = _up(np.asarray(rows, np.int64)) if rows is not None else None
        d_count = _up(np.asarray([count], np.int64)) if count is not None else None
        d_out = _up(np.asarray(out, np.float64))
        d_sub = None if sub is None else _up(np.asarray(sub, np.float64))
        rc = self.lib.tpe_joint_score_rows(
            *self._head(s), None if d_rows is None else d_rows.data_ptr(),
            None if d_count is None else d_count.data_ptr(), list_begin, max_rows,
            None if d_sub is None else d_sub.data_ptr(), d_out.data_ptr(), mode,
            self.scratch.data_ptr(), self.sp)
        t.cuda.synchronize()
        assert rc == expect, (rc, self.lib.tpe_last_error())
        assert (self.scratch[need:].cpu().numpy() == 0xA5).all()
        return d_out.cpu().numpy()


def _scorer():
    if "scorer" not in _S:
        _S["scorer"] = _Scorer()
    return _S["scorer"]


def _lists(P):
    rng = np.random.RandomState(2)
    perm = rng.permutation(P)
    return {"identity": np.arange(P), "permutation": perm, "subset": perm[:137].copy()}


@pytest.mark.parametrize("name", ["identity", "permutation", "subset"])
def test_list_scores_have_the_dense_bits(name):
    sc = _scorer()
    rows = _lists(sc.P)[name]
    for s in (0, 1):
        got = sc.call(s, rows, rows.size, 0, rows.size, 0, np.full(rows.size + GUARD, FILL))
        assert _same_bits(got[:rows.size], sc.dense[s][rows]), (name, s)
        assert (got[rows.size:] == FILL).all()


def test_list_windows_of_128():
    sc = _scorer()
    rows = _lists(sc.P)["permutation"]
    for s in (0, 1):
        for p0 in (0, 128, 256):
            got = sc.call(s, rows, rows.size, p0, 128, 0, np.full(128 + GUARD, FILL))
            k = min(128, rows.size - p0)
            assert _same_bits(got[:k], sc.dense[s][rows[p0:p0 + k]]), (s, p0)
            assert (got[k:] == FILL).all()
        # a window that starts at or past the count writes nothing
        got = sc.call(s, rows, rows.size, 384, 128, 0, np.full(128, FILL))
        assert (got == FILL).all()


@pytest.mark.parametrize("count", [0, 1, 255, 256, 257])
def test_nothing_is_written_past_the_count(count):
    sc = _scorer()
    rows = _lists(sc.P)["permutation"]  # (300 entries: the buffer is longer than the count)
    for s in (0, 1):
        got = sc.call(s, rows, count, 0, 300, 0, np.full(300, FILL))
        assert _same_bits(got[:count], sc.dense[s][rows[:count]])
        assert (got[count:] == FILL).all()
        S0 = np.full(sc.ld, FILL)
        got = sc.call(s, rows, count, 0, 300, L.JOINT_OUT_SCATTER, S0)
        want = S0.copy()
        want[rows[:count]] = sc.dense[s][rows[:count]]
        assert _same_bits(got, want)


def test_out_of_range_rows_are_skipped():
    sc = _scorer()
    rows = _lists(sc.P)["permutation"].copy()
    bad = {3: -1, 130: sc.ld, 255: 2 ** 40, 256: -2 ** 40, 299: sc.ld + 7}
    for p, r in bad.items():
        rows[p] = r
    good = np.asarray([p for p in range(rows.size) if p not in bad])
    for s in (0, 1):
        got = sc.call(s, rows, rows.size, 0, 300, 0, np.full(300, FILL))
        assert _same_bits(got[good], sc.dense[s][rows[good]])
        assert (got[list(bad)] == FILL).all()
        for mode in (L.JOINT_OUT_SCATTER, L.JOINT_OUT_SCATTER | L.JOINT_OUT_ADD):
            S0 = np.linspace(-3.0, 5.0, sc.ld)
            got = sc.call(s, rows, rows.size, 0, 300, mode, S0)
            want = S0.copy()
            with np.errstate(invalid="ignore"):
                v = sc.dense[s][rows[good]]
                want[rows[good]] = S0[rows[good]] + v if mode & L.JOINT_OUT_ADD else v
            assert _same_bits(got, want)


def test_the_three_output_modes_and_sub_by_position():
    sc = _scorer()
    rows = _lists(sc.P)["subset"]
    rng = np.random.RandomState(4)
    sub = rng.normal(size=128) * 50.0
    p0 = 5  # positions [5, 133): sub is indexed from the window's start
    k = min(128, rows.size - p0)
    listed = rows[p0:p0 + k]
    for s in (0, 1):
        with np.errstate(invalid="ignore"):
            v = sc.dense[s][listed] - sub[:k]
        got = sc.call(s, rows, rows.size, p0, 128, 0, np.full(128 + GUARD, FILL), sub=sub)
        assert _same_bits(got[:k], v) and (got[k:] == FILL).all()
        S0 = rng.normal(size=sc.ld) * 10.0
        got = sc.call(s, rows, rows.size, p0, 128, L.JOINT_OUT_SCATTER, S0, sub=sub)
        want = S0.copy()
        want[listed] = v
        assert _same_bits(got, want)                          # untouched rows keep their bits
        got = sc.call(s, rows, rows.size, p0, 128, L.JOINT_OUT_SCATTER | L.JOINT_OUT_ADD, S0,
                      sub=sub)
        want = S0.copy()
        with np.errstate(invalid="ignore"):
            want[listed] = S0[listed] + v                     # old + v, in fp64
        assert _same_bits(got, want)
    # sub = log L itself: 0 where finite, NaN where both are -inf
    dense = sc.dense[0]
    got = sc.call(0, np.arange(sc.P), sc.P, 0, sc.P, 0, np.full(sc.P, FILL), sub=dense)
    assert np.isnan(got[[5, 299]]).all() and (np.delete(got, [5, 299]) == 0.0).all()


def test_score_rows_refuses_bad_arguments():
    sc = _scorer()
    rows = np.arange(sc.P)
    out = np.full(sc.ld, FILL)

    def refused(**kw):
        a = dict(s=0, rows=rows, count=sc.P, list_begin=0, max_rows=sc.P, mode=0, out=out)
        a.update(kw)
        got = sc.call(expect=-1, **a)
        assert (got == FILL).all()                            # nothing was launched

    refused(list_begin=-1)
    refused(max_rows=-1)
    refused(mode=L.JOINT_OUT_ADD)                             # ADD needs SCATTER
    refused(mode=4)
    refused(mode=-1)
    refused(rows=None)
    refused(count=None)
    assert b"tpe_joint_score_rows" in sc.lib.tpe_last_error()
    head = list(sc._head(0))
    tail = (None, None, 0, 16, None, None, 0, None, None)
    assert sc.lib.tpe_joint_score_rows(*(head[:2] + [0] + head[3:]), *tail) == -1   # no label
    assert sc.lib.tpe_joint_score_rows(head[0], None, L.COND_MAX_LABELS + 1, *head[3:], *tail) \
        == L.E_UNSUPPORTED
    # max_rows == 0 is a no-op
    assert (sc.call(0, rows, sc.P, 0, 0, 0, out) == FILL).all()
