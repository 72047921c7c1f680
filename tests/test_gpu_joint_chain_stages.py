"""tpe_joint_chain_rows through the C ABI (csrc/tpe_joint_chain.hip): one walk
that gives log L - log L_ctx, against the two-call form -- tpe_joint_score_rows
on the same prepared set, minus tpe_joint_score_rows with n_labels = n_ctx on a
set that tpe_joint_prep builds from the first n_ctx labels with the head's
sigmas copied from the full set.  Everything is exact: bits, the positions of
NaN (-inf - -inf; a NaN's own bits are not compared) and what a call must
leave untouched (sentinel-filled buffers).

The history is synthetic: D = 6 labels in the order cont, cat, quant | cont,
quant, cat, so n_ctx = 3 has one label of every kind on either side; n_ctx = 1
and n_ctx = D - 1 are the ends.  n + 1 is 1 (the empty set), 8 and 9 (the pass
edge), 256 and 257 (the chunk edge) and 513 (three chunks).
"""
import numpy as np
import pytest

from hyperopt_amd import Domain, hp, rand, tpe
from hyperopt_amd import _lib as L
from hyperopt_amd import joint as J

pytestmark = pytest.mark.gpu

FILL = -1234.5           # what an output holds before a call
GUARD = 8
P_ROWS = 300
T_ROWS = 512
ORDER = ["c0", "k1", "q0", "c1", "q1", "k0"]
N_CTX = [1, 3, 5]
SIZES = [0, 7, 8, 255, 256, 512]   # n: n + 1 components
ZERO_ROWS = [5, 299]     # pool rows that hold k1's option of probability 0
_S = {}


def _space():
    return {"c0": hp.loguniform("c0", -2, 1), "q0": hp.quniform("q0", 0, 10, 2),
            "k0": hp.randint("k0", 5), "c1": hp.normal("c1", 1, 2),
            "q1": hp.qlognormal("q1", 0, 1, 1),
            "k1": hp.pchoice("k1", [(0.0, 0), (0.4, 1), (0.6, 2)])}


def _torch():
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    return torch, dev


def _up(a):
    t, dev = _torch()
    return t.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    """The same NaN positions, the same bits everywhere else."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and (nan == np.isnan(b)).all() and \
        (_bits(a)[~nan] == _bits(b)[~nan]).all()


class _World(object):
    """The pool and the history on the device, and per (n, n_ctx) the full
    set, the context's set and the two-call values of every pool row."""

    def __init__(self):
        t, dev = _torch()
        self.lib = L.load()
        self.eng = tpe.engine()
        self.sp = J.stream_ptr(self.eng)
        self.domain = Domain(lambda x: 0, _space())
        self.n_cols = len(self.domain.params)
        rng = np.random.RandomState(17)
        hist = tpe.Pool(self.domain, [rand.sample_config(self.domain, rng) for _ in range(T_ROWS)])
        pool = tpe.Pool(self.domain, [rand.sample_config(self.domain, rng) for _ in range(P_ROWS)])
        vals = pool.vals.copy()
        vals[ZERO_ROWS, list(self.domain.params).index("k1")] = 0.0
        self.ld = P_ROWS + GUARD
        block = np.zeros((self.n_cols, self.ld))
        block[:, :P_ROWS] = vals.T
        self.vals = _up(block)
        self.hv = _up(hist.vals.T.copy())
        self.ha = _up(np.ones((self.n_cols, T_ROWS), np.uint8))
        self.models = J.label_models(self.domain, ORDER)
        assert [m.kind for m in self.models] == [L.JOINT_CONT, L.JOINT_CAT, L.JOINT_QUANT,
                                                 L.JOINT_CONT, L.JOINT_QUANT, L.JOINT_CAT]
        self.dj = J._device_labels(self.eng, self.models, 1.0)
        self.ctx_dj = {k: J._device_labels(self.eng, self.models[:k], 1.0) for k in N_CTX}
        self.scratch = t.empty(self.lib.tpe_joint_chain_scratch_bytes(self.ld, T_ROWS) + 64,
                               dtype=t.uint8, device=dev)
        self.sets, self.two = {}, {}

    def full_set(self, n):
        if n not in self.sets:
            seen = (None, self.hv.data_ptr(), self.ha.data_ptr(), T_ROWS, None, T_ROWS)
            self.sets[n] = J._prepare_set(self.eng, self.dj, seen, self.n_cols,
                                          np.arange(n, dtype=np.int64), 25, 1.0, 0.2, self.sp)[0]
        return self.sets[n]

    def ctx_set(self, n, n_ctx):
        """tpe_joint_prep over the first n_ctx labels, the head from the full set."""
        t, dev = _torch()
        D, C = len(self.models), n + 1
        full = self.full_set(n)
        dj = self.ctx_dj[n_ctx]
        dset = t.empty(self.lib.tpe_joint_set_doubles(n_ctx, n), dtype=t.float64, device=dev)
        dset[:C].copy_(full[:C])                                      # log w
        dset[C:C + n_ctx].copy_(full[C:C + n_ctx])                    # sigma
        dset[C + n_ctx:C + 2 * n_ctx].copy_(full[C + D:C + D + n_ctx])  # 1 / (sqrt(2) sigma)
        L.check(self.lib.tpe_joint_prep(dj.host.ctypes.data, dj.dev.data_ptr(), n_ctx,
                                        self.hv.data_ptr(), self.ha.data_ptr(), T_ROWS, self.n_cols,
                                        None, n, dset.data_ptr(), self.sp), "tpe_joint_prep")
        return dset

    def _rows_call(self, dj, D, dset, n):
        t, dev = _torch()
        out = t.full((P_ROWS,), FILL, dtype=t.float64, device=dev)
        rows, count = _up(np.arange(P_ROWS, dtype=np.int64)), _up(np.asarray([P_ROWS], np.int64))
        tab = None if dj.tables is None else dj.tables.data_ptr()
        L.check(self.lib.tpe_joint_score_rows(
            dj.host.ctypes.data, dj.dev.data_ptr(), D, tab, dj.n_tables, dset.data_ptr(), n,
            self.vals.data_ptr(), self.ld, self.n_cols, rows.data_ptr(), count.data_ptr(), 0,
            P_ROWS, None, out.data_ptr(), 0, self.scratch.data_ptr(), self.sp),
            "tpe_joint_score_rows")
        return out.cpu().numpy()

    def two_call(self, n, n_ctx):
        """(full, ctx) of every pool row from tpe_joint_score_rows."""
        if (n, n_ctx) not in self.two:
            full = self._rows_call(self.dj, len(self.models), self.full_set(n), n)
            ctx = self._rows_call(self.ctx_dj[n_ctx], n_ctx, self.ctx_set(n, n_ctx), n)
            self.two[n, n_ctx] = (full, ctx)
        return self.two[n, n_ctx]

    def want(self, n, n_ctx):
        full, ctx = self.two_call(n, n_ctx)
        with np.errstate(invalid="ignore"):
            return full - ctx

    def call(self, n, n_ctx, rows, count, list_begin, max_rows, mode, out, sub=None, expect=0):
        """One tpe_joint_chain_rows call; ``out``: the output's initial
        contents (numpy).  Returns what it holds afterwards."""
        t, _dev = _torch()
        dj = self.dj
        need = self.lib.tpe_joint_chain_scratch_bytes(max_rows, n)
        self.scratch[need:].fill_(0xA5)
        d_rows, d_count = _up(np.asarray(rows, np.int64)), _up(np.asarray([count], np.int64))
        d_out = _up(np.asarray(out, np.float64))
        d_sub = None if sub is None else _up(np.asarray(sub, np.float64))
        rc = self.lib.tpe_joint_chain_rows(
            dj.host.ctypes.data, dj.dev.data_ptr(), len(self.models), n_ctx, dj.tables.data_ptr(),
            dj.n_tables, self.full_set(n).data_ptr(), n, self.vals.data_ptr(), self.ld,
            self.n_cols, d_rows.data_ptr(), d_count.data_ptr(), list_begin, max_rows,
            None if d_sub is None else d_sub.data_ptr(), d_out.data_ptr(), mode,
            self.scratch.data_ptr(), self.sp)
        t.cuda.synchronize()
        assert rc == expect, (rc, self.lib.tpe_last_error())
        assert (self.scratch[need:].cpu().numpy() == 0xA5).all()
        return d_out.cpu().numpy()


def _world():
    if "w" not in _S:
        _S["w"] = _World()
    return _S["w"]


def _perm():
    return np.random.RandomState(2).permutation(P_ROWS)


# -- 1. bit equality with the two-call form, at every set size ----------------------
@pytest.mark.parametrize("n", SIZES)
def test_one_walk_has_the_bits_of_two_calls(n):
    w = _world()
    rows = _perm()
    for n_ctx in N_CTX:
        full, ctx = w.two_call(n, n_ctx)
        want = w.want(n, n_ctx)
        # the case has what it is meant to have: k1's dead option is -inf where
        # k1 is in the group alone, NaN where the context holds it too
        assert np.isfinite(np.delete(want, ZERO_ROWS)).all()
        assert np.isneginf(full[ZERO_ROWS]).all()
        if n_ctx == 1:
            assert np.isneginf(want[ZERO_ROWS]).all()
        else:
            assert np.isneginf(ctx[ZERO_ROWS]).all() and np.isnan(want[ZERO_ROWS]).all()
        got = w.call(n, n_ctx, rows, rows.size, 0, rows.size, 0, np.full(rows.size + GUARD, FILL))
        assert _same(got[:rows.size], want[rows]), (n, n_ctx)
        assert (got[rows.size:] == FILL).all()
        again = w.call(n, n_ctx, rows, rows.size, 0, rows.size, 0, np.full(rows.size + GUARD, FILL))
        assert _same(again, got)
    if n:  # the term is not the full mixture's value, and depends on n_ctx
        assert not _same(w.want(n, 1), w.two_call(n, 1)[0])
        assert not _same(w.want(n, 1), w.want(n, 5))


# -- 2. the list ---------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 255, 256, 257])
def test_nothing_is_written_past_the_count(count):
    w = _world()
    rows = _perm()  # (300 entries: the buffer is longer than the count)
    n, n_ctx = 256, 3
    want = w.want(n, n_ctx)
    got = w.call(n, n_ctx, rows, count, 0, 300, 0, np.full(300, FILL))
    assert _same(got[:count], want[rows[:count]])
    assert (got[count:] == FILL).all()
    S0 = np.full(w.ld, FILL)
    got = w.call(n, n_ctx, rows, count, 0, 300, L.JOINT_OUT_SCATTER, S0)
    exp = S0.copy()
    exp[rows[:count]] = want[rows[:count]]
    assert _same(got, exp)


def test_a_window_that_ends_past_the_list():
    w = _world()
    rows = _perm()[:137]
    n, n_ctx = 512, 5
    want = w.want(n, n_ctx)
    got = w.call(n, n_ctx, rows, rows.size, 100, 128, 0, np.full(128 + GUARD, FILL))
    assert _same(got[:37], want[rows[100:]]) and (got[37:] == FILL).all()
    # a window that starts at or past the count writes nothing
    for begin in (137, 256):
        assert (w.call(n, n_ctx, rows, rows.size, begin, 128, 0, np.full(128, FILL)) == FILL).all()


def test_out_of_range_rows_are_skipped():
    w = _world()
    rows = _perm().copy()
    bad = {3: -1, 130: w.ld, 255: 2 ** 40, 256: -2 ** 40, 299: w.ld + 7}
    for p, r in bad.items():
        rows[p] = r
    good = np.asarray([p for p in range(rows.size) if p not in bad])
    n, n_ctx = 8, 1
    want = w.want(n, n_ctx)
    got = w.call(n, n_ctx, rows, rows.size, 0, 300, 0, np.full(300, FILL))
    assert _same(got[good], want[rows[good]])
    assert (got[list(bad)] == FILL).all()
    for mode in (L.JOINT_OUT_SCATTER, L.JOINT_OUT_SCATTER | L.JOINT_OUT_ADD):
        S0 = np.linspace(-3.0, 5.0, w.ld)
        got = w.call(n, n_ctx, rows, rows.size, 0, 300, mode, S0)
        exp = S0.copy()
        with np.errstate(invalid="ignore"):
            v = want[rows[good]]
            exp[rows[good]] = S0[rows[good]] + v if mode & L.JOINT_OUT_ADD else v
        assert _same(got, exp)


# -- 3. sub and the three output modes -------------------------------------------------
@pytest.mark.parametrize("n_ctx", N_CTX)
def test_the_three_output_modes_and_sub_by_position(n_ctx):
    w = _world()
    rows = _perm()[:137]
    rng = np.random.RandomState(4)
    sub = rng.normal(size=128) * 50.0
    p0 = 5  # positions [5, 133): sub is indexed from the window's start
    k = min(128, rows.size - p0)
    listed = rows[p0:p0 + k]
    n = 256
    with np.errstate(invalid="ignore"):
        v = w.want(n, n_ctx)[listed] - sub[:k]                # (full - ctx) first, then - sub
    got = w.call(n, n_ctx, rows, rows.size, p0, 128, 0, np.full(128 + GUARD, FILL), sub=sub)
    assert _same(got[:k], v) and (got[k:] == FILL).all()
    S0 = rng.normal(size=w.ld) * 10.0
    got = w.call(n, n_ctx, rows, rows.size, p0, 128, L.JOINT_OUT_SCATTER, S0, sub=sub)
    exp = S0.copy()
    exp[listed] = v
    assert _same(got, exp)                                    # untouched rows keep their bits
    got = w.call(n, n_ctx, rows, rows.size, p0, 128, L.JOINT_OUT_SCATTER | L.JOINT_OUT_ADD, S0,
                 sub=sub)
    exp = S0.copy()
    with np.errstate(invalid="ignore"):
        exp[listed] = S0[listed] + v                          # old + v, in fp64
    assert _same(got, exp)


def test_chain_rows_refuses_bad_arguments():
    w = _world()
    rows = np.arange(P_ROWS)
    out = np.full(w.ld, FILL)

    def refused(**kw):
        a = dict(n=8, n_ctx=3, rows=rows, count=P_ROWS, list_begin=0, max_rows=P_ROWS, mode=0,
                 out=out)
        a.update(kw)
        assert (w.call(expect=-1, **a) == FILL).all()         # nothing was launched

    for n_ctx in (0, -1, 6, 7):
        refused(n_ctx=n_ctx)
    refused(list_begin=-1)
    refused(mode=L.JOINT_OUT_ADD)
    refused(mode=4)
    assert b"tpe_joint_chain_rows" in w.lib.tpe_last_error()
    assert (w.call(8, 3, rows, P_ROWS, 0, 0, 0, out) == FILL).all()   # max_rows == 0: a no-op
