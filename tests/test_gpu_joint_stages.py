"""The joint Parzen kernels stage by stage (csrc/tpe_joint.hip: k_joint_prep,
k_joint_score, k_joint_merge), through tpe_joint_prep / tpe_joint_score on
torch tensors, against the 50-digit values of tests/golden/joint_cases.npz.

Every value is held to |got - ref| <= K_DEV * 2**-53 * cond, cond the fixture's
per-row condition number and K_DEV = 8 K_CPU rounded up to a power of two
(tests/joint_cases.py; K_CPU is measured in tests/test_joint_cases.py, which
also proves what the cases here are named for); -inf and NaN positions are
compared exactly, and so are bits wherever the kernels promise them.  Each
stage prints the largest K it measured.

The prepared set's component array is located only by what the header makes
public: it is the last 2 D (n + 1) doubles of tpe_joint_set_doubles(D, n),
{mu, constant} pairs, label-major.
"""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _lib as L
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from hyperopt_amd import tpe
from tests import joint_cases as JC

pytestmark = pytest.mark.gpu

GUARD = 8                 # doubles on either side of an output
FILL = -1234.5            # what a buffer holds before a kernel writes it
_DEV = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.shape(a) == np.shape(b) and (_bits(a) == _bits(b)).all()


class _Case(object):
    """A case's inputs on the device."""

    def __init__(self, case, pool_rows=None, ld=None, hist_pad=5):
        import torch
        self.t, self.lib, self.case = torch, L.load(), case
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.host = np.ascontiguousarray(case["labels"])
        self.D = len(self.host)
        self.labels = self._up(self.host.view(np.uint8))
        tabs = [np.concatenate(J.cat_tables(m, case["smoothing"]))
                for m in JC.models_of(case) if m.kind == L.JOINT_CAT]
        self.n_tables = sum(t.size for t in tabs)
        self.tables = self._up(np.concatenate(tabs)) if tabs else None
        # the history, label-major, its leading dimension larger than its rows
        N, self.n_cols = case["hist"].shape
        self.hld = N + hist_pad
        hv = np.full((self.n_cols, self.hld), np.nan)
        hv[:, :N] = case["hist"].T
        self.hvals = self._up(hv)
        self.hact = self._up(np.ones((self.n_cols, self.hld), np.uint8))
        pool = case["pool"] if pool_rows is None else case["pool"][pool_rows]
        self.P = pool.shape[0]
        self.ld = self.P if ld is None else ld
        pv = np.full((self.n_cols, self.ld), np.nan)
        pv[:, :self.P] = pool.T
        self.pool = self._up(pv)
        self.sp = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _up(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def head(self, s):
        c = self.case
        n = c["sets"][s].size
        sig = c["sig"][s]
        some = sig > 0.0  # (as joint._prepare_set: 0, never an infinity, for no bandwidth)
        r = np.where(some, 1.0 / (np.sqrt(2.0) * np.where(some, sig, 1.0)), 0.0)
        return np.concatenate([J.log_weights(n, c["lf"], c["prior_weight"]), sig, r])

    def prep(self, s, head=None, null_rows=False):
        """The prepared set s as a tensor of tpe_joint_set_doubles + GUARD doubles."""
        t, c = self.t, self.case
        rows = c["sets"][s]
        n = int(rows.size)
        total = self.lib.tpe_joint_set_doubles(self.D, n)
        assert total >= (n + 1) + 2 * self.D + 2 * self.D * (n + 1)
        dset = t.full((total + GUARD,), FILL, dtype=t.float64, device=self.dev)
        head = self.head(s) if head is None else head
        dset[:head.size].copy_(t.from_numpy(head))
        drows = None if null_rows else self._up(np.asarray(rows, np.int32))
        L.check(self.lib.tpe_joint_prep(self.host.ctypes.data, self.labels.data_ptr(), self.D,
                                        self.hvals.data_ptr(), self.hact.data_ptr(), self.hld,
                                        self.n_cols, None if drows is None else drows.data_ptr(),
                                        n, dset.data_ptr(), self.sp), "tpe_joint_prep")
        t.cuda.synchronize()
        return dset, n, total

    def score(self, dset, n, row_begin=0, n_rows=None, sub=None):
        """(out with its guards, scratch with its guard) of one tpe_joint_score call."""
        t = self.t
        n_rows = self.P if n_rows is None else n_rows
        out = t.full((n_rows + 2 * GUARD,), FILL, dtype=t.float64, device=self.dev)
        need = self.lib.tpe_joint_scratch_bytes(n_rows, n)
        assert need == 16 * n_rows * ((n + 1 + 255) // 256)
        scratch = t.full((need + 64,), 0xA5, dtype=t.uint8, device=self.dev)
        tab = None if self.tables is None else self.tables.data_ptr()
        L.check(self.lib.tpe_joint_score(self.host.ctypes.data, self.labels.data_ptr(), self.D,
                                         tab, self.n_tables, dset.data_ptr(), n,
                                         self.pool.data_ptr(), self.ld, self.n_cols, row_begin,
                                         n_rows, None if sub is None else sub.data_ptr(),
                                         out.data_ptr() + 8 * GUARD, scratch.data_ptr(), self.sp),
                "tpe_joint_score")
        t.cuda.synchronize()
        out, tail = out.cpu().numpy(), scratch[need:].cpu().numpy()
        assert (out[:GUARD] == FILL).all() and (out[GUARD + n_rows:] == FILL).all()
        assert (tail == 0xA5).all()
        return out[GUARD:GUARD + n_rows]

    def log_l(self, s):
        dset, n, _ = self.prep(s)
        return self.score(dset, n)


def _dev(name):
    assert L.load().tpe_joint_chunk() == 256  # the cases' geometry is this constant's
    if name not in _DEV:
        _DEV[name] = _Case(JC.load()[name])
    return _DEV[name]


def _check(stage, items):
    """items: (what, got, ref, cond); asserts each within K_DEV, prints the stage's largest K."""
    worst, at = 0.0, None
    for what, got, ref, cond in items:
        k = JC.k_of(got, ref, cond)
        if k > worst:
            worst, at = k, what
    print("%s: device max K = %.3g at %s (K_DEV = %g)" % (stage, worst, at, JC.K_DEV))
    assert worst <= JC.K_DEV, (stage, at, worst)


# -- 1. prep -----------------------------------------------------------------------
def test_prep_read_back():
    """mu and the constant per (label, component) for n in {0, 7, 8, 255, 256},
    rows permuted (rows = NULL at n = 0), history values of 0.0 and 1e-13 on
    the log kinds, a randint stored as 12.0 .. 24.0."""
    dc = _dev("prep")
    c, lab, D = dc.case, dc.case["labels"], dc.D
    items = []
    for s, n in enumerate(JC.PREP_N):
        head = dc.head(s)
        dset, n_, total = dc.prep(s, null_rows=(n == 0))
        assert n_ == n
        got = dset.cpu().numpy()
        C = n + 1
        assert _same_bits(got[:head.size], head)                    # the head: untouched
        off = total - 2 * D * C
        assert off >= head.size and (got[head.size:off] == FILL).all()  # (the pad, if any)
        assert (got[total:] == FILL).all()                          # nothing past the set
        comp = got[off:total].reshape(D, C, 2)
        mu, cst = comp[:, :, 0], comp[:, :, 1]
        ref_mu, ref_cst, cond = c["prep_mu"][s], c["prep_cst"][s], c["prep_cond"][s]
        for d in range(D):
            what = "n=%d label %d" % (n, d)
            is_log = bool(lab["flags"][d] & L.JOINT_LOG)
            obs = c["hist"][c["sets"][s], lab["col"][d]]
            if lab["kind"][d] == L.JOINT_CAT:
                if lab["shift"][d] == 12 and n:
                    assert obs.min() >= 12.0 and obs.max() <= 24.0
                assert _same_bits(mu[d], np.concatenate([obs - lab["shift"][d], [-1.0]])), what
                assert _same_bits(cst[d], np.zeros(C)), what
                continue
            if not is_log:
                assert _same_bits(mu[d], np.concatenate([obs, [lab["prior_mu"][d]]])), what
            else:
                assert _same_bits(mu[d, n], lab["prior_mu"][d])
                items.append((what + " mu", mu[d], ref_mu[d], 1.0 + np.abs(ref_mu[d])))
            assert np.isfinite(ref_cst[d]).all()
            items.append((what + " cst", cst[d], ref_cst[d], cond[d].astype(np.float64)))
    _check("prep", items)


# -- 2. score ----------------------------------------------------------------------
def _score_items(names):
    items = []
    for name in names:
        dc = _dev(name)
        for s in range(len(dc.case["sets"])):
            items.append(("%s set %d" % (name, s), dc.log_l(s), dc.case["logl"][s],
                          dc.case["cond"][s]))
    return items


@pytest.mark.parametrize("C", JC.GEO_C)
def test_score_geometry(C):
    """The prior at every place of a pass; C = 0 and 1 mod 256; one and three
    chunks; a last pass that is full, ragged, or the prior alone."""
    _check("score geo%d" % C, _score_items(["geo%d" % C]))


@pytest.mark.parametrize("C", JC.ONEHOT_C)
def test_score_one_hot(C):
    """log w = 0 at one component and -inf elsewhere: log L is that a_i."""
    dc = _dev("geo%d" % C)
    c = dc.case
    items = []
    for j, i in enumerate(c["onehot"]):
        head = dc.head(0)
        head[:C] = -np.inf
        head[i] = 0.0
        dset, n, _ = dc.prep(0, head=head)
        items.append(("component %d" % i, dc.score(dset, n), c["onehot_a"][j],
                      c["onehot_cond"][j]))
    _check("one-hot C=%d" % C, items)


@pytest.mark.parametrize("name", ["run_up", "run_down", "run_mid"])
def test_score_running_maximum(name):
    _check(name, _score_items([name]))


@pytest.mark.parametrize("name", ["dead_chunks", "dead_passes"])
def test_score_dead_chunks_and_passes(name):
    dc = _dev(name)
    got = dc.log_l(0)
    assert np.isfinite(got[:30]).all() and np.isneginf(got[30:]).all()
    _check(name, [(name, got, dc.case["logl"][0], dc.case["cond"][0])])
    # sub = -inf where log L is: NaN, as the pool code ranks it
    dset, n, _ = dc.prep(0)
    sub = dc._up(got)
    out = dc.score(dset, n, sub=sub)
    assert np.isnan(out[30:]).all() and (out[:30] == 0.0).all()


@pytest.mark.parametrize("name", ["edge_qlognormal", "edge_qloguniform", "edge_quniform",
                                  "edge_lognormal", "edge_pchoice"])
def test_score_factor_edges_and_sub(name):
    dc = _dev(name)
    lb, la = dc.log_l(0), dc.log_l(1)
    c = dc.case
    _check(name, [("below", lb, c["logl"][0], c["cond"][0]),
                  ("above", la, c["logl"][1], c["cond"][1])])
    # out with sub has the bits of numpy's log L - sub; NaN where both are -inf
    dset, n, _ = dc.prep(0)
    out = dc.score(dset, n, sub=dc._up(la))
    with np.errstate(invalid="ignore"):
        want = lb - la
    assert _same_bits(out, want)
    np.testing.assert_array_equal(np.isnan(out),
                                  np.isneginf(c["logl"][0]) & np.isneginf(c["logl"][1]))


@pytest.mark.parametrize("D", JC.LABEL_COUNTS)
def test_score_label_counts(D):
    """The tile staging loop runs once (ragged, then full), twice and four times;
    columns permuted, the unused ones NaN in pool and history."""
    _check("labels%d" % D, _score_items(["labels%d" % D]))


def test_score_prep_case_sets():
    """The prep history's five sets scored too (every kind, empty set included)."""
    _check("prep sets", _score_items(["prep"]))


# -- 3. windows --------------------------------------------------------------------
def test_windows_keep_the_bits_and_stay_inside_their_buffers():
    case = JC.load()["geo513"]
    tiled = np.arange(520) % JC.P
    dc = _Case(case, pool_rows=tiled, ld=600)
    dset, n, _ = dc.prep(0)
    whole = dc.score(dset, n, 0, 520)
    assert _same_bits(whole, _dev("geo513").log_l(0)[tiled])
    _check("windows", [("whole", whole, case["logl"][0][tiled], case["cond"][0][tiled])])
    for r0 in (0, 1, 255, 256, 257):
        for k in (1, 255, 256, 257):
            assert r0 + k <= 520
            assert _same_bits(dc.score(dset, n, r0, k), whole[r0:r0 + k]), (r0, k)


# -- 4. the public path ------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(JC.PUBLIC))
def test_public_path(name):
    c = JC.load()[name]
    domain, trials, rows, kw = JC.public_problem(c)
    pool = tpe.Pool(domain, rows)
    S, terms, Jd = tpe.score_configs(domain, trials, pool, joint=True, return_terms=True, **kw)
    assert _same_bits(S, Jd) and np.isnan(terms).all()
    st = pool_mod._settings(kw["prior_weight"], kw["gamma"], kw["linear_forgetting"], True,
                            kw["bandwidth"], kw["cat_smoothing"])
    _eng, d = pool_mod._score_device(domain, trials, pool, st, False, want_parts=True)
    lb, la, j2 = d.parts[:, :JC.P].cpu().numpy()
    assert _same_bits(j2, Jd) and _same_bits(lb - la, Jd)
    _check(name, [("below", lb, c["logl"][0], c["cond"][0]),
                  ("above", la, c["logl"][1], c["cond"][1]),
                  ("J", Jd, c["logl"][0] - c["logl"][1], c["cond"][0] + c["cond"][1])])
    # and the C entry points on the same sets: the same bits
    dc = _dev(name)
    assert _same_bits(dc.log_l(0), lb) and _same_bits(dc.log_l(1), la)


# -- 5. the all-kinds case of test_gpu_joint.py --------------------------------------
def test_all_kinds_case_against_50_digits():
    from tests.test_gpu_joint import KW, P_ROWS, _all_kinds
    c = JC.load()["all_kinds"]
    domain, trials, pool, _ = _all_kinds()
    hist = tpe.collect_history(trials, pool.labels)
    assert _same_bits(np.asarray(hist.vals, np.float64), c["hist"])   # the fixture's inputs
    ids = c["row_ids"]
    assert ids.size == JC.P and {5, 150, 299} <= set(ids.tolist())
    shift = np.zeros(pool.vals.shape[1])
    shift[c["labels"]["col"]] = c["labels"]["shift"]
    assert _same_bits(np.asarray(pool.vals, np.float64)[ids] - shift[None, :], c["pool"])
    st = pool_mod._settings(KW["prior_weight"], KW["gamma"], KW["linear_forgetting"], True,
                            KW["bandwidth"], KW["cat_smoothing"])
    _eng, d = pool_mod._score_device(domain, trials, pool, st, False, want_parts=True)
    lb, la, _ = d.parts[:, :P_ROWS].cpu().numpy()
    _check("all kinds", [("below", lb[ids], c["logl"][0], c["cond"][0]),
                         ("above", la[ids], c["logl"][1], c["cond"][1])])
