"""The resident history stage by stage through the C ABI: tpe_history_append,
tpe_history_order, tpe_fit_sorted, tpe_gather_obs and tpe_gather_obs_multi
(csrc/tpe_history.hip, csrc/tpe_sorted.hip) against the numpy restatements of
tests/history_cases.py, on the cases of that file -- the appended block at 255
and 256 threads, new rows around the LDS sort's powers of two and old rows
around the merge's blocks, value classes (ties, +-0.0, infinities, NaN, clamped
logs), the fit's chunk counts and rank words at its chunk edges on both the
local and the globalize path, the gathers at their pass edges.  Chunk, pass and
new-row sizes come from tpe_fit_sorted_layout.

Every buffer a call may write starts as 0xA5 bytes between two guards of 64
such bytes, the scratch included; what the reference does not name must still
be 0xA5 afterwards.  Orders, lists, counts and words are compared exactly;
the fitted mixtures with oracle.adaptive_parzen_normal at the tolerances of
tests/test_gpu_sorted_fit.py, and bit for bit with tpe_gather_obs +
tpe_parzen_fit on the same history.

Slips made one at a time in the kernel source on a scratch build fail here:
`<` and `<=` swapped in either search of k_order_merge (test_order, the ties
of every size and value case with old rows; test_order_in_pieces); the index
tie-break of k_order_sort_new dropped (test_order: equal, two, new-in-run,
zeros, nan, log-clamped, log-nonpositive and the tied size cases); the ramp by
sorted position (test_fit: reverse, all, several and the rest with a ramp).
`first` from chunk 0 alone, a gather without its carry or without its count
guard would read or write out of bounds, so they are not run: they are
restated on the host in tests/test_history_cases.py, which shows the cases
here that differ (last-row beyond one chunk; every list with members in two
passes; count-short-*).
"""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _lib as L
from oracle import tpe_oracle as O
from tests import history_cases as HC

pytestmark = pytest.mark.gpu

GUARD = 64       # bytes on either side of a buffer that must stay as they were
POISON = 0xA5
E_ARG = -1
PRIOR_POS0 = 12345   # a segment's prior_pos before a call


@pytest.fixture(scope="module")
def gpu():
    import torch
    lib = L.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    return _Gpu(torch, lib, dev)


class _Gpu(object):
    def __init__(self, torch, lib, dev):
        self.t, self.lib, self.dev = torch, lib, dev

    @property
    def stream(self):
        return ctypes.c_void_p(self.t.cuda.current_stream(self.dev).cuda_stream)

    def sync(self):
        self.t.cuda.synchronize(self.dev)

    def buf(self, nbytes, data=None, zero=False):
        return _Buf(self, nbytes, data, zero)

    def of(self, arr):
        arr = np.ascontiguousarray(arr)
        return _Buf(self, arr.nbytes, arr)


class _Buf(object):
    """nbytes device bytes between two guards, all POISON (or zero, or data)."""

    def __init__(self, g, nbytes, data=None, zero=False):
        self.g, self.n = g, int(nbytes)
        host = np.full(self.n + 2 * GUARD, POISON, np.uint8)
        if zero:
            host[GUARD:GUARD + self.n] = 0
        if data is not None:
            raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
            host[GUARD:GUARD + raw.size] = raw
        self.t = g.t.from_numpy(host).to(g.dev)
        self.ptr = self.t.data_ptr() + GUARD
        assert self.ptr % 8 == 0

    def put(self, arr, byte_off=0):
        raw = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        assert 0 <= byte_off and byte_off + raw.size <= self.n
        lo = GUARD + byte_off
        self.t[lo:lo + raw.size].copy_(self.g.t.from_numpy(raw.copy()))

    def get(self, dtype=np.uint8):
        """The payload; the guards must be intact."""
        host = self.t.cpu().numpy()
        assert (host[:GUARD] == POISON).all(), "bytes before the buffer were written"
        assert (host[GUARD + self.n:] == POISON).all(), "bytes after the buffer were written"
        return host[GUARD:GUARD + self.n].copy().view(dtype)


def _poison(n, dtype):
    return np.full(n * np.dtype(dtype).itemsize, POISON, np.uint8).view(dtype)


def _same_bytes(got, want, msg=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, msg
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8))
        item = got.dtype.itemsize
        raise AssertionError("%s: %d elements differ, first at %d: %r != %r" % (
            msg, np.unique(bad // item).size, bad[0] // item, got.reshape(-1)[bad[0] // item],
            want.reshape(-1)[bad[0] // item]))


# ---------------------------------------------------------------------------
# stage 1: tpe_history_append
# ---------------------------------------------------------------------------
def _append(gpu, stage, nl, k, V, A, ld, r0):
    rc = gpu.lib.tpe_history_append(stage.ptr if stage is not None else None, nl, k, V.ptr, A.ptr,
                                    ld, r0, gpu.stream)
    gpu.sync()
    return rc


@pytest.mark.parametrize("c", HC.APPEND, ids=lambda c: c.name)
def test_append(gpu, c):
    sv, sa = HC.append_stage(c)
    stage = gpu.of(np.concatenate([sv.reshape(-1).view(np.uint8), sa.reshape(-1)]))
    V, A = gpu.buf(8 * c.n_labels * c.ld), gpu.buf(c.n_labels * c.ld)
    assert _append(gpu, stage, c.n_labels, c.k, V, A, c.ld, c.r0) == 0
    want_v = _poison(c.n_labels * c.ld, np.float64).reshape(c.n_labels, c.ld)
    want_a = _poison(c.n_labels * c.ld, np.uint8).reshape(c.n_labels, c.ld)
    HC.append_ref(want_v, want_a, sv, sa, c.r0)
    _same_bytes(V.get(np.float64).reshape(c.n_labels, c.ld), want_v, "vals")
    _same_bytes(A.get().reshape(c.n_labels, c.ld), want_a, "active")


def test_append_nothing_and_errors(gpu):
    stage, V, A = gpu.buf(64), gpu.buf(8 * 3 * 10), gpu.buf(3 * 10)
    for nl, k, ld, r0, want in ((3, 0, 10, 2, 0), (0, 4, 10, 2, 0), (3, 4, 5, 2, E_ARG),
                                (3, 4, 10, 7, E_ARG), (3, 4, 10, -1, E_ARG), (-1, 4, 10, 0, E_ARG),
                                (3, -1, 10, 0, E_ARG)):
        assert _append(gpu, stage, nl, k, V, A, ld, r0) == want, (nl, k, ld, r0)
        if want:
            assert b"tpe_history_append" in gpu.lib.tpe_last_error()
    assert (V.get() == POISON).all() and (A.get() == POISON).all()


# ---------------------------------------------------------------------------
# stage 2: tpe_history_order
# ---------------------------------------------------------------------------
class _Order(object):
    """A history of n_cols columns under ld, its order matrix (all POISON) and
    the scratch of tpe_history_order for `specs` [(col, transform, floor)]."""

    def __init__(self, gpu, vals, ld, specs):
        self.g, self.ld, self.specs = gpu, ld, specs
        self.n_cols, self.rows = vals.shape
        host = _poison(self.n_cols * ld, np.float64).reshape(self.n_cols, ld)
        host[:, :self.rows] = vals
        self.V = gpu.of(host)
        self.O = gpu.buf(4 * self.n_cols * ld)
        self.arr = np.zeros(len(specs), L.COLSPEC_DTYPE)
        if specs:
            self.arr["col"], self.arr["transform"], self.arr["floor"] = zip(*specs)
        self.dspecs = gpu.of(self.arr.view(np.uint8)) if specs else gpu.buf(16)
        self.S = gpu.buf(gpu.lib.tpe_history_order_scratch_bytes(len(specs), self.rows))

    def seed(self, col, order):
        self.O.put(np.asarray(order, np.int32), 4 * col * self.ld)

    def step(self, n_old, n_new, n_specs=None, ld=None):
        rc = self.g.lib.tpe_history_order(self.V.ptr, self.ld if ld is None else ld,
                                          self.dspecs.ptr, self.arr.ctypes.data,
                                          len(self.specs) if n_specs is None else n_specs,
                                          n_old, n_new, self.O.ptr, self.S.ptr, self.g.stream)
        self.g.sync()
        return rc

    def order(self):
        self.S.get()   # (the scratch's guards)
        return self.O.get(np.int32).reshape(self.n_cols, self.ld)


def _check_order(got, key, n, msg):
    np.testing.assert_array_equal(got[:n], HC.order_ref(key[:n]), err_msg=msg)
    assert (got[n:] == _poison(1, np.int32)[0]).all(), msg + ": written beyond the rows"


@pytest.mark.parametrize("c", HC.ORDER, ids=lambda c: c.name)
def test_order(gpu, c):
    key = HC.tkey(c.v, c.transform, c.floor)
    run = _Order(gpu, c.v[None, :], c.ld, [(0, c.transform, c.floor)])
    run.seed(0, HC.order_ref(key[:c.n_old]))
    assert run.step(c.n_old, c.n_new) == 0
    _check_order(run.order()[0], key, c.n_old + c.n_new, c.name)
    _same_bytes(run.V.get(np.float64)[:key.size], np.asarray(c.v), "the values")


@pytest.mark.parametrize("schedule", sorted(HC.PIECES))
def test_order_in_pieces(gpu, schedule):
    """5000 rows of two columns (identity; log with clamped ties) ordered in
    pieces: after every piece the stable argsort of the rows so far."""
    vals, specs = HC.pieces_columns()
    keys = [HC.tkey(vals[col], tr, floor) for col, tr, floor in specs]
    run = _Order(gpu, vals, HC.PIECES_ROWS + 7, specs)
    n = 0
    for k in HC.PIECES[schedule]:
        assert run.step(n, k) == 0
        n += k
        got = run.order()
        for (col, _, _), key in zip(specs, keys):
            _check_order(got[col], key, n, "%s: column %d at %d rows" % (schedule, col, n))
    assert n == HC.PIECES_ROWS


def test_order_of_several_specs(gpu):
    """Specs for columns {2, 0} of four: the other columns' orders, the entries
    beyond the rows and the bytes around the scratch stay as they were."""
    vals, specs, n_old, n_new, ld = HC.multi_spec_case()
    run = _Order(gpu, vals, ld, specs)
    keys = {col: HC.tkey(vals[col], tr, floor) for col, tr, floor in specs}
    for col, key in keys.items():
        run.seed(col, HC.order_ref(key[:n_old]))
    assert run.step(n_old, n_new) == 0
    got = run.order()
    for col, key in keys.items():
        _check_order(got[col], key, n_old + n_new, "column %d" % col)
    assert (got[[1, 3]] == _poison(1, np.int32)[0]).all()


def test_order_nothing_and_errors(gpu):
    vals = np.random.RandomState(1).normal(size=(2, HC.NEW + 1))
    run = _Order(gpu, vals, HC.NEW + 1, [(0, HC.IDENT, 0.0), (1, HC.LOG, 0.5)])
    assert run.step(0, HC.NEW + 1) == E_ARG       # more new rows than one call takes
    assert b"tpe_history_order" in gpu.lib.tpe_last_error()
    assert run.step(HC.NEW - 5, 7) == E_ARG       # n_old + n_new > ld
    assert run.step(0, 5, ld=4) == E_ARG
    assert run.step(-1, 5) == E_ARG and run.step(0, -1) == E_ARG
    run.arr["transform"][1] = 7                    # a bad transform
    assert run.step(0, 5) == E_ARG
    run.arr["transform"][1] = HC.LOG
    run.arr["col"][0] = -1
    assert run.step(0, 5) == E_ARG
    run.arr["col"][0] = 0
    assert run.step(10, 0) == 0 and run.step(0, 5, n_specs=0) == 0   # nothing to do
    assert (run.order().view(np.uint8) == POISON).all()
    assert (run.S.get() == POISON).all()


# ---------------------------------------------------------------------------
# stage 3: tpe_fit_sorted
# ---------------------------------------------------------------------------
POOLS = (("w", 8), ("mu", 8), ("sigma", 8), ("wcdf", 8), ("coef64", 32), ("coef32", 16))
GAP = 2   # components left between two segments' windows


class _Fit(object):
    """A fit case on the device: history, flags, descriptors and segments
    (component windows GAP apart), and the numpy orders of its columns."""

    def __init__(self, gpu, c):
        self.g, self.c = gpu, c
        self.n_cols, self.N = c.vals.shape
        self.ld = self.N + (5 if self.N % 2 else 0)   # (ld == n_rows for the even sizes)
        v = _poison(self.n_cols * self.ld, np.float64).reshape(self.n_cols, self.ld)
        a = _poison(self.n_cols * self.ld, np.uint8).reshape(self.n_cols, self.ld)
        v[:, :self.N], a[:, :self.N] = c.vals, c.active
        self.V, self.A = gpu.of(v), gpu.of(a)
        self.isb = HC.is_below(c)
        self.IS = gpu.of(self.isb)
        self.replays = [HC.fit_replay(c, s) for s in c.segs]
        orders = _poison(self.n_cols * self.ld, np.int32).reshape(self.n_cols, self.ld)
        self.col_spec = {}
        for s in c.segs:
            spec = (s.col, s.transform, s.floor)
            assert self.col_spec.setdefault(s.col, spec) == spec
            orders[s.col, :self.N] = HC.order_ref(HC.seg_key(c, s))
        self.orders = orders
        counts = np.array([r.n + s.claim for r, s in zip(self.replays, c.segs)], np.int64)
        self.counts, n_seg = counts, len(c.segs)
        self.obs_off = np.cumsum(counts) - counts
        self.comp_off = np.cumsum(counts + 1 + GAP) - (counts + 1 + GAP) + 1
        self.n_obs_total, self.n_comp = int(counts.sum()), int((counts + 1 + GAP).sum()) + 1
        self.max_obs = int(counts.max())
        g = np.zeros(n_seg, L.GATHER_DTYPE)
        g["col"], g["below"] = [s.col for s in c.segs], [s.below for s in c.segs]
        g["dst_off"], g["count"] = self.obs_off, counts
        sg = np.zeros(n_seg, L.SEG_DTYPE)
        sg["obs_off"], sg["comp_off"], sg["n_obs"] = self.obs_off, self.comp_off, counts
        for name in ("lf", "transform", "floor", "prior_weight", "prior_mu", "prior_sigma", "low",
                     "high", "bounded"):
            sg[name] = [getattr(s, name) for s in c.segs]
        sg["family"] = [HC.LGMM1 if s.transform == HC.LOG else HC.GMM1 for s in c.segs]
        sg["prior_pos"] = PRIOR_POS0
        self.g_arr, self.segs = g, sg
        self.G = gpu.of(g.view(np.uint8))

    def pools(self):
        return {name: self.g.buf(size * self.n_comp) for name, size in POOLS}

    def sorted_fit(self, order=None):
        """(pools, segs read back, scratch bytes, err) of one tpe_fit_sorted."""
        g, lib, n_seg = self.g, self.g.lib, len(self.c.segs)
        OR = g.of(self.orders) if order is None else order
        S = g.of(self.segs.view(np.uint8))
        ws = g.buf(lib.tpe_fit_sorted_scratch_bytes(n_seg, self.N))
        err = g.buf(16, zero=True)
        P = self.pools()
        rc = lib.tpe_fit_sorted(self.V.ptr, self.A.ptr, self.ld, OR.ptr, self.N, self.IS.ptr,
                                self.G.ptr, self.g_arr.ctypes.data, S.ptr, n_seg, ws.ptr,
                                *[P[name].ptr for name, _ in POOLS], err.ptr, g.stream)
        g.sync()
        assert rc == 0, lib.tpe_last_error()
        if order is None:
            _same_bytes(OR.get(np.int32), self.orders.reshape(-1), "the order")
        return ({k: b.get() for k, b in P.items()}, S.get().view(L.SEG_DTYPE), ws.get(),
                int(err.get(np.int32)[0]))

    def sort_fit(self):
        """(pools, segs read back, err) of tpe_gather_obs + tpe_parzen_fit."""
        g, lib, n_seg = self.g, self.g.lib, len(self.c.segs)
        S = g.of(self.segs.view(np.uint8))
        obs = g.buf(8 * max(self.n_obs_total, 1))
        err = g.buf(16, zero=True)
        rc = lib.tpe_gather_obs(self.V.ptr, self.A.ptr, self.ld, None, self.N, self.IS.ptr,
                                self.G.ptr, self.g_arr.ctypes.data, n_seg, obs.ptr, None, err.ptr,
                                g.stream)
        assert rc == 0, lib.tpe_last_error()
        ws = g.buf(lib.tpe_fit_scratch_bytes(n_seg, self.max_obs, self.n_obs_total))
        P = self.pools()
        rc = lib.tpe_parzen_fit(obs.ptr, ws.ptr, S.ptr, n_seg, self.max_obs, self.n_obs_total,
                                *[P[name].ptr for name, _ in POOLS], None, None, None, None,
                                g.stream)
        g.sync()
        assert rc == 0, lib.tpe_last_error()
        ws.get()
        # (the gathered lists while they are here)
        got = obs.get(np.float64)
        for s, r, o in zip(self.c.segs, self.replays, self.obs_off):
            np.testing.assert_array_equal(got[o:o + r.n], self.c.vals[s.col][r.member])
        return {k: b.get() for k, b in P.items()}, S.get().view(L.SEG_DTYPE), \
            int(err.get(np.int32)[0])

    def windows(self, pool, size):
        """Per segment the bytes of its component window; and the rest."""
        mask = np.zeros(pool.size, bool)
        out = []
        for off, n in zip(self.comp_off, self.counts):
            lo, hi = size * int(off), size * int(off + n + 1)
            out.append(pool[lo:hi])
            mask[lo:hi] = True
        return out, pool[~mask]


def _check_scratch(run, raw, globalized):
    """Chunk counts and rank words of every segment against the replay."""
    N, n_seg = run.N, len(run.c.segs)
    lay = HC.layout(n_seg, N)
    gi, cnt, part, total = lay[:4]
    assert raw.size == total and lay[4] == HC.CHUNK and lay[5] == HC.CNT
    nch = max(1, (N + HC.CHUNK - 1) // HC.CHUNK)
    words = raw[gi:gi + 4 * n_seg * N].copy().view(np.int32).reshape(n_seg, N)
    counts = raw[cnt:cnt + 4 * HC.CNT * n_seg * nch].copy().view(np.int32).reshape(n_seg, nch, HC.CNT)
    for i, r in enumerate(run.replays):
        msg = "%s segment %d" % (run.c.name, i)
        np.testing.assert_array_equal(counts[i], r.cnt, err_msg=msg + ": chunk counts")
        np.testing.assert_array_equal(words[i], r.glob if globalized else r.local,
                                      err_msg=msg + ": rank words")
    # between the regions nothing is written
    assert (raw[gi + 4 * n_seg * N:cnt] == POISON).all()
    assert (raw[cnt + 4 * HC.CNT * n_seg * nch:part] == POISON).all()


def _check_mixtures(run, pools, segs):
    c = run.c
    for name, size in POOLS:
        _, rest = run.windows(pools[name], size)
        assert (rest == POISON).all(), "%s: %s written outside the windows" % (c.name, name)
    W = {name: [w.copy().view(np.float64) for w in run.windows(pools[name], 8)[0]]
         for name in ("w", "mu", "sigma")}
    for i, (s, r) in enumerate(zip(c.segs, run.replays)):
        msg = "%s segment %d" % (c.name, i)
        obs = HC.seg_lists(c, s)
        ow, omu, osig = O.adaptive_parzen_normal(obs, s.prior_weight, s.prior_mu, s.prior_sigma,
                                                 s.lf)
        gw, gmu, gsig = W["w"][i], W["mu"][i], W["sigma"][i]
        assert int(segs["prior_pos"][i]) == r.prior_pos, msg
        assert omu[r.prior_pos] == s.prior_mu and osig[r.prior_pos] == s.prior_sigma
        if s.transform == HC.LOG:
            np.testing.assert_allclose(gmu, omu, rtol=4.5e-16, atol=0, err_msg=msg)
        else:
            np.testing.assert_array_equal(gmu, omu, err_msg=msg)
        np.testing.assert_allclose(gsig, osig, rtol=1e-12, atol=0, err_msg=msg)
        np.testing.assert_allclose(gw, ow, rtol=1e-12, atol=0, err_msg=msg)


@pytest.mark.parametrize("N", HC.FIT_ROWS)
def test_fit(gpu, N, monkeypatch):
    for c in HC.size_cases("fit", N):
        run = _Fit(gpu, c)
        ref_pools, ref_segs, ref_err = run.sort_fit()
        assert ref_err == 0
        for env in ("0", "1"):
            monkeypatch.setenv("TPE_FIT_GLOBALIZE", env)
            pools, segs, raw, err = run.sorted_fit()
            assert err == 0, c.name
            _check_scratch(run, raw, env == "1")
            _check_mixtures(run, pools, segs)
            # bit for bit the gather + sort fit, pools and segment records
            for name, _ in POOLS:
                _same_bytes(pools[name], ref_pools[name], "%s env=%s %s" % (c.name, env, name))
            _same_bytes(segs.view(np.uint8), ref_segs.view(np.uint8), c.name + " segments")


def test_fit_from_the_device_order(gpu, monkeypatch):
    """tpe_history_order's own output (built in three calls) into
    tpe_fit_sorted: the bits of the fit from the uploaded numpy order."""
    monkeypatch.setenv("TPE_FIT_GLOBALIZE", "0")
    N = 2 * HC.CHUNK + 1
    c = [x for x in HC.size_cases("fit", N) if x.name.endswith("several")][0]
    run = _Fit(gpu, c)
    specs = sorted(run.col_spec.values())
    od = _Order(gpu, np.asarray(c.vals), run.ld, specs)
    n = 0
    for k in (1000, 1, N - 1001):
        assert od.step(n, k) == 0
        n += k
    got = od.order()
    for col, _, _ in specs:
        np.testing.assert_array_equal(got[col, :N], run.orders[col, :N])
    a = run.sorted_fit(order=od.O)
    b = run.sorted_fit()
    assert a[3] == b[3] == 0
    for name, _ in POOLS:
        _same_bytes(a[0][name], b[0][name], name)
    _same_bytes(a[1].view(np.uint8), b[1].view(np.uint8), "segments")
    _same_bytes(a[2][:HC.layout(len(c.segs), N)[2]], b[2][:HC.layout(len(c.segs), N)[2]], "scratch")
    _check_mixtures(run, a[0], a[1])


@pytest.mark.parametrize("env", ["0", "1"])
@pytest.mark.parametrize("delta", [-1, 1])
def test_fit_count_mismatch(gpu, delta, env, monkeypatch):
    """The middle segment of three claims count + delta: bit 4 of err, its
    windows untouched, nothing outside the pools' windows touched."""
    monkeypatch.setenv("TPE_FIT_GLOBALIZE", env)
    c = HC.mismatch_case(delta)
    run = _Fit(gpu, c)
    pools, segs, raw, err = run.sorted_fit()
    assert err & 4
    for name, size in POOLS:
        wins, rest = run.windows(pools[name], size)
        assert (rest == POISON).all(), name
        # (w and mu by the compaction, the rest by the fit's tail, which skips
        # a segment the compaction flagged)
        assert (wins[1] == POISON).all(), "%s of the mismatched segment was written" % name
    # its record is as the host gave it: a scorer launched before the host
    # reads err still finds a prior_pos inside the segment's window
    _same_bytes(segs[1:2].view(np.uint8), run.segs[1:2].view(np.uint8), "the mismatched segment")
    assert int(segs["prior_pos"][0]) == run.replays[0].prior_pos
    # the chunk counts still say what was found
    lay = HC.layout(3, run.N)
    nch = (run.N + HC.CHUNK - 1) // HC.CHUNK
    counts = raw[lay[1]:lay[1] + 4 * HC.CNT * 3 * nch].copy().view(np.int32).reshape(3, nch, HC.CNT)
    assert int(counts[1, :, 0].sum()) == run.replays[1].n == run.counts[1] - delta


def test_fit_nothing_and_errors(gpu):
    c = HC.size_cases("fit", 2)[0]
    run = _Fit(gpu, c)
    lib, P = gpu.lib, run.pools()
    S, OR = gpu.of(run.segs.view(np.uint8)), gpu.of(run.orders)
    ws = gpu.buf(lib.tpe_fit_sorted_scratch_bytes(len(c.segs), run.N))

    def call(n_seg, n_rows, g_arr=run.g_arr):
        rc = lib.tpe_fit_sorted(run.V.ptr, run.A.ptr, run.ld, OR.ptr, n_rows, run.IS.ptr, run.G.ptr,
                                g_arr.ctypes.data, S.ptr, n_seg, ws.ptr,
                                *[P[name].ptr for name, _ in POOLS], None, gpu.stream)
        gpu.sync()
        return rc
    assert call(0, run.N) == 0
    assert call(-1, run.N) == E_ARG and call(1, run.ld + 1) == E_ARG and call(1, -1) == E_ARG
    bad = run.g_arr.copy()
    bad["count"][0] = run.N + 1
    assert call(len(c.segs), run.N, bad) == E_ARG
    bad = run.g_arr.copy()
    bad["to_int"][0] = 1
    assert call(len(c.segs), run.N, bad) == E_ARG
    assert b"tpe_fit_sorted" in lib.tpe_last_error()
    for b in list(P.values()) + [ws]:
        assert (b.get() == POISON).all()


# ---------------------------------------------------------------------------
# stage 4: tpe_gather_obs, tpe_gather_obs_multi
# ---------------------------------------------------------------------------
WGAP = 3   # words between two descriptors' windows


def _windows(cases_descs):
    """dst_off of every (case, descriptor) in two pools (fp64, int64), windows
    of max(matches, count) slots WGAP apart; the expected pools; the lists."""
    offs, refs = [], []
    size = {0: WGAP, 1: WGAP}
    for c, d in cases_descs:
        ref = HC.gather_ref(c, d)
        count = ref.size if d.count is None else d.count
        offs.append(size[d.to_int])
        refs.append((ref, count))
        size[d.to_int] += max(ref.size, count) + WGAP
    want = {0: _poison(size[0], np.float64), 1: _poison(size[1], np.int64)}
    for (c, d), off, (ref, count) in zip(cases_descs, offs, refs):
        k = min(ref.size, count)
        want[d.to_int][off:off + k] = ref[:k]
    return offs, refs, want


def _g_arr(cases_descs, offs, refs):
    g = np.zeros(len(cases_descs), L.GATHER_DTYPE)
    for i, ((c, d), off, (ref, count)) in enumerate(zip(cases_descs, offs, refs)):
        g[i] = (d.col, d.below, off, d.offset, count, d.to_int, d.hist)
    return g


def _gather(gpu, c, with_err=True):
    """One tpe_gather_obs call over the case's descriptors: the two pools
    (compared with the reference here) and err."""
    lib = gpu.lib
    cd = [(c, d) for d in c.descs]
    offs, refs, want = _windows(cd)
    g = _g_arr(cd, offs, refs)
    V, A, IS, G = gpu.of(c.vals), gpu.of(c.active), gpu.of(c.is_below), gpu.of(g.view(np.uint8))
    R = gpu.of(c.rows) if c.rows is not None else None
    F, I = gpu.buf(8 * want[0].size), gpu.buf(8 * want[1].size)
    err = gpu.buf(16, zero=True)
    rc = lib.tpe_gather_obs(V.ptr, A.ptr, c.vals.shape[1], R.ptr if R is not None else None,
                            c.is_below.size, IS.ptr, G.ptr, g.ctypes.data, len(g), F.ptr, I.ptr,
                            err.ptr if with_err else None, gpu.stream)
    gpu.sync()
    assert rc == 0, lib.tpe_last_error()
    got = {0: F.get(np.float64), 1: I.get(np.int64)}
    for k in (0, 1):
        _same_bytes(got[k], want[k], "%s: %s pool" % (c.name, ("fp64", "int64")[k]))
    for b, src in ((V, c.vals), (A, c.active), (IS, c.is_below)):
        _same_bytes(b.get(src.dtype), np.ascontiguousarray(src).reshape(-1), c.name + ": an input")
    e = int(err.get(np.int32)[0])
    assert (err.get(np.int32)[1:] == 0).all()
    mismatch = any(ref.size != count for ref, count in refs)
    if with_err:
        assert e == (4 if mismatch else 0), c.name
    return got, offs, refs


@pytest.mark.parametrize("N", HC.GATHER_ROWS)
def test_gather_sizes(gpu, N):
    for c in HC.size_cases("gather", N):
        _gather(gpu, c)


@pytest.mark.parametrize("c", HC.GATHER_SPECIAL, ids=lambda c: c.name)
def test_gather_descriptors(gpu, c):
    _gather(gpu, c)


def test_gather_without_err(gpu):
    _gather(gpu, HC.GATHER_SPECIAL_BY_NAME["several"], with_err=False)


def test_gather_multi(gpu):
    """Three histories of different ld and length in one launch, descriptors
    interleaved across them: the reference's lists, and the bytes
    tpe_gather_obs writes for the same descriptor alone."""
    lib = gpu.lib
    hs, launch = HC.multi_case()
    cd = [(hs[h], hs[h].descs[i]) for h, i in launch]
    offs, refs, want = _windows(cd)
    g = _g_arr(cd, offs, refs)
    # aux: per history the flags, then (4-aligned) the row list
    aux, H, keep = [], np.zeros(len(hs), L.HISTORY_DTYPE), []
    size = 0
    for h, c in enumerate(hs):
        V, A = gpu.of(c.vals), gpu.of(c.active)
        keep += [V, A]
        isb_off, size = size, size + (c.is_below.size + 3) // 4 * 4
        aux.append(np.resize(c.is_below, size - isb_off))
        rows_off = -1
        if c.rows is not None:
            rows_off, size = size, size + 4 * c.rows.size
            aux.append(c.rows.view(np.uint8))
        H[h] = (V.ptr, A.ptr, c.vals.shape[1], c.vals.shape[0], c.is_below.size, rows_off, isb_off)
    AUX, HD, G = gpu.of(np.concatenate(aux)), gpu.of(H.view(np.uint8)), gpu.of(g.view(np.uint8))
    F, I = gpu.buf(8 * want[0].size), gpu.buf(8 * want[1].size)
    err = gpu.buf(16, zero=True)
    rc = lib.tpe_gather_obs_multi(HD.ptr, H.ctypes.data, len(hs), AUX.ptr, G.ptr, g.ctypes.data,
                                  len(g), F.ptr, I.ptr, err.ptr, gpu.stream)
    gpu.sync()
    assert rc == 0, lib.tpe_last_error()
    got = {0: F.get(np.float64), 1: I.get(np.int64)}
    for k in (0, 1):
        _same_bytes(got[k], want[k], "multi: %s pool" % ("fp64", "int64")[k])
    assert int(err.get(np.int32)[0]) == 0
    # every descriptor alone through tpe_gather_obs
    for h, c in enumerate(hs):
        single, s_offs, s_refs = _gather(gpu, c)
        for i, d in enumerate(c.descs):
            j = launch.index((h, i))
            n = s_refs[i][0].size
            assert n == refs[j][0].size
            _same_bytes(got[d.to_int][offs[j]:offs[j] + n],
                        single[d.to_int][s_offs[i]:s_offs[i] + n], "history %d descriptor %d" % (h, i))
