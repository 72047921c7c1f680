"""The liar batch's kernels (csrc/tpe_joint_lie.hip) through the C ABI,
tpe_joint_lie_picks on torch tensors with synthetic S_0 / A_0 / values, against
the scalar restatement in tests/liar_util.py.

Tolerance.  S_0, A_0 and log W are inputs, so S_k = S_0 - (U_k - U_0) carries
the error of U_k alone, and U_0 = log W + A_0 is one exact fp64 add on both
sides: |S_k - ref| <= 1e-6 (|U_0| + |U_k|), the project's fp64 log-density
tolerance (1e-6 relative per log-density: test_gpu_parity.py, test_gpu_joint.py).
Picks: synthetic scores of 600 rows lie closer together than any tolerance, so
the restatement follows the device's picks (``forced``) and reports, per pick,
how much better its own choice would have been; that regret is held to the same
bound -- 0 wherever the two agree, which the test prints.  Twins (equal values,
S_0 and A_0) keep equal bits on both sides and are told apart by row order
alone.  -inf / NaN positions, inputs, guards and bits across pool shapes are
compared exactly.
"""
import ctypes
import math

import numpy as np
import pytest

from hyperopt_amd import Domain, hp, tpe
from hyperopt_amd import _lib as L
from hyperopt_amd import joint as J
from tests import joint_util as U
from tests import liar_util as LU

pytestmark = pytest.mark.gpu

E_ARG = -1
GUARD = 8
FILL = -1234.5
ROW_FILL = -77
SMOOTHING = 0.5
LOG_W, LOG_LIE = math.log(12.5), math.log(0.8)
SPACES = {
    # one label of each factor kind: bounded log continuous, unbounded
    # quantized log, categorical with an option of probability zero
    "kinds": lambda: {"u": hp.loguniform("u", -2, 1), "v": hp.qlognormal("v", 0, 1, 0.5),
                      "w": hp.pchoice("w", [(0.0, 0), (0.3, 1), (0.7, 2)])},
    "one": lambda: {"x": hp.normal("x", 0, 1)},  # D = 1
}
SIGMA = {"kinds": [0.3, 0.4, 0.0], "one": [0.25]}
_SHARED = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.shape(a) == np.shape(b) and (_bits(a) == _bits(b)).all()


def _inputs(space, P, seed=0):
    """Synthetic pool values (P, D), S_0, A_0 and masks.  Past P = 1: NaN and
    -0.0 / +0.0 scores, an A_0 of -inf (U_0 is not finite: S stays S_0), a
    lower edge <= 0 on the quantized label, rows of the probability-zero
    option (a lie of another option is -inf there), full twins, and half the
    rows taken or masked."""
    rng = np.random.RandomState(1000 * seed + P)
    if space == "kinds":
        X = np.stack([np.exp(rng.uniform(-2, 1, P)), 0.5 * rng.randint(0, 13, P),
                      rng.choice(3, P, p=[0.2, 0.3, 0.5]).astype(np.float64)], 1)
    else:
        X = rng.normal(0, 1, (P, 1))
    S0 = rng.normal(0, 1, P)
    A0 = rng.uniform(-6, 2, P)
    taken = (rng.uniform(size=P) < 0.4).astype(np.uint8)
    distinct = (rng.uniform(size=P) < 0.15).astype(np.uint8)
    if P > 8:
        S0[[3, P - 1]] = np.nan
        S0[4], S0[6] = -0.0, 0.0
        A0[7] = -np.inf
        for a, b in ((1, P - 2), (2, 5)):  # full twins
            X[b], S0[b], A0[b] = X[a], S0[a], A0[a]
        S0[2] = S0[5] = 4.0                # ... one pair the best real score of all
        taken[[1, 2, 3, 4, 5, 6, P - 2, P - 1]] = 0
        distinct[[1, 2, 3, 4, 5, 6, P - 2, P - 1]] = 0
    else:
        taken[:], distinct[:] = 0, 0
    return X, S0, A0, taken, distinct


class _Dev(object):
    """A space's labels on the device, and one call of tpe_joint_lie_picks."""

    def __init__(self, space):
        import torch
        self.t, self.lib, self.eng = torch, L.load(), tpe.engine()
        self.dev = self.eng.device
        domain = Domain(lambda x: 0, SPACES[space]())
        self.names = list(domain.params)
        self.models = J.label_models(domain)
        self.dj = J._device_labels(self.eng, self.models, SMOOTHING)
        self.infos = [U.label_info(domain.specs[lab]) for lab in self.names]
        self.D = len(self.models)
        sig = np.asarray(SIGMA[space])
        some = sig > 0.0
        self.sig_host = np.concatenate([sig, np.where(some, 1.0 / (np.sqrt(2.0) * np.where(
            some, sig, 1.0)), 0.0)])
        self.sigma = self.up(self.sig_host)
        self.sp = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def up(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def tab(self):
        return None if self.dj.tables is None else self.dj.tables.data_ptr()

    def picks(self, X, S0, A0, taken, distinct, k, ld_pad=3, trace=True):
        """(rows, S_at_pick, S_k, count) of one call; guards and inputs checked."""
        t = self.t
        P = X.shape[0]
        ld = P + ld_pad
        pv = np.full((self.D, ld), np.nan)
        pv[:, :P] = X.T
        d_vals, d_S0, d_A0 = self.up(pv), self.up(S0), self.up(A0)
        d_taken = self.up(taken)
        d_dist = None if distinct is None else self.up(distinct)
        kk = max(k, 1)
        rows = t.full((kk + 2 * GUARD,), ROW_FILL, dtype=t.int64, device=self.dev)
        count = t.full((3,), ROW_FILL, dtype=t.int64, device=self.dev)
        at = t.full((kk + 2 * GUARD,), FILL, dtype=t.float64, device=self.dev)
        S_k = t.full((P + 2 * GUARD,), FILL, dtype=t.float64, device=self.dev)
        need = self.lib.tpe_joint_lie_scratch_bytes(P)
        assert need >= 25 * P and need % 16 == 0
        scratch = t.full((need + 64,), 0xA5, dtype=t.uint8, device=self.dev)
        rc = self.lib.tpe_joint_lie_picks(
            self.dj.host.ctypes.data, self.dj.dev.data_ptr(), self.D, self.tab(),
            self.dj.n_tables, self.sigma.data_ptr(), d_vals.data_ptr(), ld, self.D, P,
            d_S0.data_ptr(), d_A0.data_ptr(), LOG_W, LOG_LIE, d_taken.data_ptr(),
            None if d_dist is None else d_dist.data_ptr(), k, rows.data_ptr() + 8 * GUARD,
            count.data_ptr() + 8, at.data_ptr() + 8 * GUARD if trace else None,
            S_k.data_ptr() + 8 * GUARD if trace else None, scratch.data_ptr(), self.sp)
        L.check(rc, "tpe_joint_lie_picks")
        t.cuda.synchronize()
        # the caller's arrays are read only
        assert _same_bits(d_vals.cpu().numpy(), pv)
        assert _same_bits(d_S0.cpu().numpy(), S0) and _same_bits(d_A0.cpu().numpy(), A0)
        assert (d_taken.cpu().numpy() == taken).all()
        assert d_dist is None or (d_dist.cpu().numpy() == distinct).all()
        assert _same_bits(self.sigma.cpu().numpy(), self.sig_host)
        cnt = count.cpu().numpy()
        assert cnt[0] == ROW_FILL and cnt[2] == ROW_FILL
        n = int(cnt[1])
        assert 0 <= n <= min(max(k, 0), P)
        rows, at, S_k = rows.cpu().numpy(), at.cpu().numpy(), S_k.cpu().numpy()
        assert (rows[:GUARD] == ROW_FILL).all() and (rows[GUARD + n:] == ROW_FILL).all()
        assert (at[:GUARD] == FILL).all() and (at[GUARD + (n if trace else 0):] == FILL).all()
        assert (S_k[:GUARD] == FILL).all() and (S_k[GUARD + (P if trace else 0):] == FILL).all()
        assert (scratch[need:].cpu().numpy() == 0xA5).all()
        return rows[GUARD:GUARD + n], at[GUARD:GUARD + n], S_k[GUARD:GUARD + P], n

    def reference(self, X, S0, A0, gone, k, forced=None):
        return LU.lie_picks(self.infos, [[float(v) for v in row] for row in X], S0, A0,
                            [float(s) for s in self.sig_host[:self.D]], LOG_W, LOG_LIE,
                            SMOOTHING, k, gone, forced)


def _dev(space):
    if space not in _SHARED:
        _SHARED[space] = _Dev(space)
    return _SHARED[space]


def _check(dc, X, S0, A0, taken, distinct, k, what):
    P = X.shape[0]
    gone = taken if distinct is None else taken | distinct
    rows, at, S_k, n = dc.picks(X, S0, A0, taken, distinct, k)
    ref = dc.reference(X, S0, A0, gone, k, forced=rows)
    assert n == min(max(k, 0), int((gone == 0).sum())), what  # every free row, or k of them
    assert len(set(rows.tolist())) == n and not gone[rows].any(), what
    assert len(ref["rows"]) == n and ref["regret"].shape == (n,), what
    bound = 1e-6 * (np.abs(ref["U_0"]) + np.abs(ref["U_k"]))
    fin = np.isfinite(bound)
    worst = bound[fin].max() if fin.any() else 0.0
    print("%s: %d picks, %d the restatement's own, max regret %.3g (bound %.3g)"
          % (what, n, int((ref["regret"] == 0.0).sum()), ref["regret"].max() if n else 0.0,
             worst))
    assert (ref["regret"] <= worst).all(), what
    # NaN scores go first, in row order
    nan_free = [r for r in np.flatnonzero(np.isnan(S0)) if not gone[r]][:n]
    assert rows[:len(nan_free)].tolist() == nan_free, what
    # S at each pick and after the last, under the same pick sequence
    np.testing.assert_array_equal(np.isnan(S_k), np.isnan(ref["S_k"]))
    np.testing.assert_array_equal(np.isnan(at), np.isnan(ref["S_at_pick"]))
    ok = ~np.isnan(S_k)
    err = np.abs(S_k[ok] - ref["S_k"][ok])
    assert (err <= np.where(fin, bound, 0.0)[ok]).all(), (what, err.max())
    okp = ~np.isnan(at)
    assert (np.abs(at[okp] - ref["S_at_pick"][okp]) <=
            np.where(fin, bound, 0.0)[rows[okp]]).all(), what
    # where U_0 is not finite, and where no lie has mass, S keeps S_0's bits
    still = ~fin | (_bits(ref["U_k"]) == _bits(ref["U_0"]))
    assert _same_bits(S_k[still], S0[still]), what
    if n:
        assert _same_bits(at[:1], S0[rows[:1]]), what  # the first pick: at S_0
    return rows, at, S_k


@pytest.mark.parametrize("P", [1, 255, 256, 257, 600])
def test_picks_and_scores_match_scalar_restatement(P):
    dc = _dev("kinds")
    X, S0, A0, taken, distinct = _inputs("kinds", P)
    for k in (1, 3, P + 2):
        rows, _at, _S_k = _check(dc, X, S0, A0, taken, distinct, k, "P=%d k=%d" % (P, k))
        if P > 8:
            assert rows[:min(k, 2)].tolist() == [3, P - 1][:min(k, 2)]  # the NaN rows
        if P > 8 and k > P:
            # twins keep equal bits pick after pick: the smaller row goes first
            at = {int(r): j for j, r in enumerate(rows)}
            assert at[2] < at[5] and at[1] < at[P - 2]
    if P > 8:
        # without the distinct mask; without traces the rows are the same
        rows, _at, _S_k = _check(dc, X, S0, A0, taken, None, 5, "P=%d no mask" % P)
        bare = dc.picks(X, S0, A0, taken, None, 5, trace=False)
        assert bare[0].tolist() == rows.tolist() and bare[3] == 5


@pytest.mark.parametrize("P", [1, 257])
def test_one_label(P):
    dc = _dev("one")
    X, S0, A0, taken, distinct = _inputs("one", P, seed=1)
    for k in (1, 3, P + 2):
        _check(dc, X, S0, A0, taken, distinct, k, "D=1 P=%d k=%d" % (P, k))


def test_bits_do_not_depend_on_the_pool_shape():
    """The 600-row pool's S_k at 257 of its rows equals, bit for bit, the S_k of
    those rows packed into a pool of their own under the same pick sequence."""
    dc = _dev("kinds")
    X, S0, A0, taken, distinct = _inputs("kinds", 600)
    gone = taken | distinct
    rows, at, S_k, n = dc.picks(X, S0, A0, taken, distinct, 6)
    assert n == 6
    rest = np.setdiff1d(np.arange(600), rows)
    sub = np.sort(np.concatenate([rows, np.random.RandomState(9).permutation(rest)[:251]]))
    assert sub.size == 257
    rows2, at2, S_k2, n2 = dc.picks(X[sub], S0[sub], A0[sub], taken[sub], distinct[sub], 6)
    assert n2 == 6 and sub[rows2].tolist() == rows.tolist()  # a best row stays best in a subset
    assert _same_bits(S_k2, S_k[sub]) and _same_bits(at2, at)
    assert not _same_bits(S_k[~np.isnan(S0)], S0[~np.isnan(S0)])
    # ... and on the leading dimension, and on a second call
    again = dc.picks(X, S0, A0, taken, distinct, 6, ld_pad=0)
    assert again[0].tolist() == rows.tolist() and _same_bits(again[2], S_k)
    assert not gone[rows].any()


def test_count_zero_cases():
    dc = _dev("kinds")
    X, S0, A0, taken, distinct = _inputs("kinds", 40)
    for k in (0, -3):
        rows, at, S_k, n = dc.picks(X, S0, A0, taken, distinct, k)
        assert n == 0 and _same_bits(S_k, S0)
    rows, at, S_k, n = dc.picks(X, S0, A0, np.ones(40, np.uint8), None, 4)
    assert n == 0 and _same_bits(S_k, S0)            # every row taken
    rows, at, S_k, n = dc.picks(X, S0, A0, taken, 1 - taken, 4)
    assert n == 0                                     # the two masks cover the pool
    rows, at, S_k, n = dc.picks(X[:0], S0[:0], A0[:0], taken[:0], None, 4, ld_pad=1)
    assert n == 0                                     # P == 0


def test_bad_arguments_return_e_arg():
    dc = _dev("kinds")
    t, lib = dc.t, dc.lib
    P = 16
    X, S0, A0, taken, distinct = _inputs("kinds", P)
    vals = dc.up(np.ascontiguousarray(X.T))
    d = dict(S0=dc.up(S0), A0=dc.up(A0), taken=dc.up(taken))
    rows = t.full((4,), ROW_FILL, dtype=t.int64, device=dc.dev)
    count = t.full((1,), ROW_FILL, dtype=t.int64, device=dc.dev)
    scratch = t.empty(lib.tpe_joint_lie_scratch_bytes(P), dtype=t.uint8, device=dc.dev)
    assert lib.tpe_joint_lie_scratch_bytes(-1) == -1

    def call(**kw):
        a = dict(host=dc.dj.host.ctypes.data, labels=dc.dj.dev.data_ptr(), D=dc.D, tab=dc.tab(),
                 n_tables=dc.dj.n_tables, sigma=dc.sigma.data_ptr(), vals=vals.data_ptr(), ld=P,
                 n_cols=dc.D, P=P, S0=d["S0"].data_ptr(), A0=d["A0"].data_ptr(), log_w=LOG_W,
                 log_lie=LOG_LIE, taken=d["taken"].data_ptr(), distinct=None, k=4,
                 rows=rows.data_ptr(), count=count.data_ptr(), scratch=scratch.data_ptr())
        a.update(kw)
        return lib.tpe_joint_lie_picks(a["host"], a["labels"], a["D"], a["tab"], a["n_tables"],
                                       a["sigma"], a["vals"], a["ld"], a["n_cols"], a["P"],
                                       a["S0"], a["A0"], a["log_w"], a["log_lie"], a["taken"],
                                       a["distinct"], a["k"], a["rows"], a["count"], None, None,
                                       a["scratch"], dc.sp)

    bad_col = dc.dj.host.copy()
    bad_col["col"][1] = dc.D
    for kw in (dict(D=0), dict(host=None), dict(P=-1), dict(ld=P - 1), dict(n_cols=dc.D - 1),
               dict(host=bad_col.ctypes.data), dict(n_tables=dc.dj.n_tables - 1),
               dict(labels=None), dict(tab=None), dict(sigma=None), dict(vals=None),
               dict(S0=None), dict(A0=None), dict(taken=None), dict(rows=None), dict(count=None),
               dict(scratch=None), dict(log_lie=float("inf")), dict(log_lie=float("-inf")),
               dict(log_lie=float("nan")), dict(log_w=float("nan")), dict(log_w=float("inf"))):
        assert call(**kw) == E_ARG, kw
        assert lib.tpe_last_error()
    t.cuda.synchronize()
    assert int(count.item()) == ROW_FILL and (rows.cpu().numpy() == ROW_FILL).all()  # no launch
    assert call() == 0
    t.cuda.synchronize()
    assert int(count.item()) == 4
