"""TPE over a fixed pool of configurations: rank the rows, suggest the best.

    pool = tpe.Pool(domain, configs)            # or Pool.from_arrays(domain, vals, active)
    fmin(fn, space, algo=partial(tpe.suggest_from_pool, pool=pool), max_queue_len=8, ...)

``tpe.suggest`` draws its candidates from the product space.  A pool holds
configurations the caller already has -- the legal tile / unroll combinations
of a kernel, the rows of a tabular benchmark, the survivors of a feasibility
check -- and ranks them with the same posteriors: for a configuration ``c``

    S(c) = sum over the labels live in c of  log l(c_label) - log g(c_label)

with l / g the below / above posteriors ``tpe.suggest`` fits for the history
(same split, linear forgetting, prior weight, per-label observations;
build_posterior, tpe.py:697-746).  On a free product space the per-label
argmax of broadcast_best (tpe.py:649-658) is the argmax of this sum, so S is
the reference's criterion for a whole configuration.  The k best rows not yet
handed out are k distinct documents, which a repeated ``tpe.suggest`` on an
unchanged history cannot give.

Device path: the pool lives in HBM, one contiguous fp64 column per label; each
column is scored in place by the exact fp64 scorers (as injected candidates,
``Engine.run(cand_ptr=...)``), in label chunks that bound the scratch space;
``tpe_pool_fold`` sums the live labels' terms per row and ``tpe_pool_topk``
selects the first k untaken rows (csrc/tpe_pool.hip).  Conditional labels are
scored for every row (an inactive entry holds a copy of one of the column's
live values) and masked in the fold.  Only the k row indices come back.
"""
from __future__ import annotations

import ctypes
import logging
import math
import time

import numpy as np

from . import _lib as _L
from .base import as_domain
from .engine import CONTINUOUS, _params
from .walk import INT_KINDS, int_offset, trial_docs

logger = logging.getLogger(__name__)

# log-densities kept on the device per engine run: a chunk holds as many labels
# as fit (at least one), so the scratch is 2 x 8 x max(P, CHUNK_ELEMS) bytes
CHUNK_ELEMS = 1 << 24


def _bounds(spec):
    """(low, high, high is excluded, values are whole numbers) of a label's
    stored values.  Quantized kinds get half a step beyond their bounds: the
    prior itself rounds across them (qloguniform(0, 3, 2) draws 0 < exp(0))."""
    k, a = spec.kind, spec.args
    if k in ("uniform", "quniform", "loguniform", "qloguniform"):
        lo, hi = float(a[0]), float(a[1])
        if "log" in k:
            lo, hi = math.exp(lo), math.exp(hi)
        if k.startswith("q"):
            lo, hi = lo - 0.5 * float(a[2]), hi + 0.5 * float(a[2])
        return lo, hi, False, False
    if k == "randint":
        lo, hi = (0, int(a[0])) if (len(a) < 2 or a[1] is None) else (int(a[0]), int(a[1]))
        return float(lo), float(hi), True, True
    if k == "categorical":
        p = np.asarray(a[0])
        return 0.0, float(p.shape[-1]), True, True
    return -math.inf, math.inf, False, False  # normal kinds: any finite value


def _switch_value(spec, v):
    return int(round(v)) if spec.kind in INT_KINDS else float(v)


def _validate(domain, labels, vals, active):
    """Raise ValueError naming the row and the label of the first invalid entry:
    every live value finite and inside its prior's support, and every row's
    label set the one its own choices make live (``domain.reachable``)."""
    P = vals.shape[0]
    for j, lab in enumerate(labels):
        spec = domain.specs[lab]
        a, v = active[:, j], vals[:, j]
        lo, hi, hi_open, whole = _bounds(spec)
        with np.errstate(invalid="ignore"):
            bad = a & ~np.isfinite(v)
            what = "is not finite"
            if not bad.any():
                bad = a & ((v < lo) | ((v >= hi) if hi_open else (v > hi)))
                what = "is outside %s%g, %g%s of %s" % ("[", lo, hi, ")" if hi_open else "]",
                                                        spec.kind)
            if not bad.any() and whole:
                bad = a & (v != np.round(v))
                what = "is not a whole number (%s)" % spec.kind
        if bad.any():
            r = int(np.flatnonzero(bad)[0])
            raise ValueError("pool row %d, label %r: value %r %s" % (r, lab, float(v[r]), what))
    if P == 0:
        return
    # the live set depends on the values of the switch selectors only: one
    # reachable() per distinct selector assignment, compared with its rows
    domain.reachable({})
    sel = getattr(domain, "_selector_labels", None)
    sel = list(labels) if sel is None else [lab for lab in sel if lab in labels]
    js = [labels.index(lab) for lab in sel]
    if js:
        keys = np.where(active[:, js], vals[:, js], -np.inf)
        uniq, inverse = np.unique(keys, axis=0, return_inverse=True)
        inverse = np.asarray(inverse).reshape(-1)
    else:
        uniq, inverse = np.zeros((1, 0)), np.zeros(P, np.int64)
    for u in range(uniq.shape[0]):
        decided = {lab: _switch_value(domain.specs[lab], uniq[u, i])
                   for i, lab in enumerate(sel) if uniq[u, i] != -np.inf}
        live = set(domain.reachable(decided))
        want = np.fromiter((lab in live for lab in labels), bool, len(labels))
        rows = np.flatnonzero(inverse == u)
        diff = active[rows] != want
        if diff.any():
            i, j = np.argwhere(diff)[0]
            raise ValueError("pool row %d, label %r: %s" % (
                int(rows[i]), labels[j],
                "missing, but live under the row's choices" if want[j]
                else "given, but not live under the row's choices"))


class _DevicePool(object):
    """A pool's mirror on one device: values (L, P) fp64 -- label j's column at
    element j * P, randint(low, high) columns offset-free as the scorers take
    them --, activity (L, P) bytes, the taken mask, and per label the
    (min, max) of its live values in the scoring coordinate."""
    __slots__ = ("vals", "active", "taken", "taken_current", "ranges", "S", "terms", "rows_out",
                 "count", "scratch")


class Pool(object):
    """A fixed set of configurations of ``domain`` to search (module doc).

    ``configs``: a sequence of {label: stored value} dicts holding exactly the
    labels live under their own choices, values as they stand in a trial's
    ``misc["vals"]`` (choice index; randint(low, high) with ``low`` included).
    Validated once (ValueError names the row and the label); quantized values
    need not lie on their lattice.  ``taken`` (uint8 per row) marks the rows
    handed out: ``mark_taken`` / ``release`` change it, ``row_of`` maps the tid
    of a suggested trial to its row.  The device copy is made at the first
    scoring and kept.
    """

    def __init__(self, domain, configs):
        domain = as_domain(domain)
        labels = list(domain.params)
        index = {lab: j for j, lab in enumerate(labels)}
        vals = np.full((len(configs), len(labels)), np.nan)
        active = np.zeros(vals.shape, bool)
        for r, cfg in enumerate(configs):
            for lab, v in cfg.items():
                j = index.get(lab)
                if j is None:
                    raise ValueError("pool row %d, label %r: not a label of the space" % (r, lab))
                try:
                    vals[r, j] = float(v)
                except (TypeError, ValueError):
                    raise ValueError("pool row %d, label %r: value %r is not a number"
                                     % (r, lab, v)) from None
                active[r, j] = True
        self._setup(domain, labels, vals, active)

    @classmethod
    def from_arrays(cls, domain, vals, active):
        """The pool of ``vals`` / ``active``: (P, L) arrays in ``domain.params``
        column order, the layout of ``walk.docs_matrix`` (entries of inactive
        labels are ignored).  For large pools."""
        domain = as_domain(domain)
        labels = list(domain.params)
        vals = np.array(vals, dtype=np.float64, ndmin=2)
        active = np.array(active, dtype=bool, ndmin=2)
        if vals.shape != active.shape or vals.shape[1] != len(labels):
            raise ValueError("vals %s / active %s: expected (P, %d)"
                             % (vals.shape, active.shape, len(labels)))
        vals[~active] = np.nan
        self = cls.__new__(cls)
        self._setup(domain, labels, vals, active)
        return self

    def _setup(self, domain, labels, vals, active):
        _validate(domain, labels, vals, active)
        self.domain, self.labels = domain, labels
        self.vals, self.active = vals, active
        self.n_active = active.sum(0)
        self.taken = np.zeros(vals.shape[0], np.uint8)
        self.row_of = {}
        self._device = {}

    def __len__(self):
        return self.vals.shape[0]

    @property
    def n_untaken(self):
        return int(len(self) - np.count_nonzero(self.taken))

    def _rows(self, rows):
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        if rows.size and (rows.min() < 0 or rows.max() >= len(self)):
            raise IndexError("pool rows outside [0, %d)" % len(self))
        return rows

    def mark_taken(self, rows):
        """Rows that are no longer to be suggested (e.g. evaluated elsewhere)."""
        self.taken[self._rows(rows)] = 1
        for d in self._device.values():
            d.taken_current = False

    def release(self, rows):
        """Rows that may be suggested again; their ``row_of`` entries go."""
        rows = self._rows(rows)
        self.taken[rows] = 0
        gone = set(rows.tolist())
        for tid in [t for t, r in self.row_of.items() if r in gone]:
            del self.row_of[tid]
        for d in self._device.values():
            d.taken_current = False

    def config(self, row):
        """Row ``row`` as the {live label: stored value} dict of a trial."""
        specs = self.domain.specs
        out = {}
        for j in np.flatnonzero(self.active[row]):
            lab = self.labels[j]
            v = self.vals[row, j]
            out[lab] = int(round(v)) if specs[lab].kind in INT_KINDS else float(v)
        return out

    # -- device mirror ---------------------------------------------------------
    def device(self, eng):
        """The pool's mirror on ``eng``'s device, uploaded once."""
        d = self._device.get(eng.device)
        t = eng.torch
        if d is None:
            P, nl = self.vals.shape
            cols = np.empty((nl, max(P, 1)))
            ranges = []
            for j, lab in enumerate(self.labels):
                spec = self.domain.specs[lab]
                a = self.active[:, j]
                c = self.vals[:, j] - (int_offset(spec) or 0)
                live = c[a]
                # (an inactive entry is scored too and masked in the fold: it
                # holds a value the scorer accepts)
                cols[j, :P] = np.where(a, c, live[0] if live.size else 0.0)
                rng = (0.0, 0.0)
                if spec.kind in CONTINUOUS and live.size:
                    if _params(spec.kind, spec.args)["family"] == _L.LGMM1:
                        with np.errstate(all="ignore"):
                            live = np.log(live)
                    live = live[np.isfinite(live)]
                    mu = _params(spec.kind, spec.args)["prior_mu"]
                    rng = (float(live.min()), float(live.max())) if live.size else (mu, mu)
                ranges.append(rng)
            d = _DevicePool()
            d.vals = t.from_numpy(cols).to(eng.device)
            d.active = t.from_numpy(np.ascontiguousarray(self.active.T).view(np.uint8)
                                    if P else np.zeros((nl, 1), np.uint8)).to(eng.device)
            d.taken = t.zeros(max(P, 1), dtype=t.uint8, device=eng.device)
            d.taken_current = False
            d.ranges = ranges
            d.S = t.empty(max(P, 1), dtype=t.float64, device=eng.device)
            d.terms = None
            d.rows_out = d.count = d.scratch = None
            self._device[eng.device] = d
        if not d.taken_current:
            d.taken[:len(self)].copy_(t.from_numpy(self.taken))
            d.taken_current = True
        return d


def _history_inputs(domain, trials, gamma, hist=None):
    """The history and level inputs exactly as tpe.suggest's _open_study makes
    them (pending and failed trials carry +inf and sit in the above set)."""
    from . import tpe as T
    labels = list(domain.params)
    if hist is None:
        hist = T.collect_history(trials, labels)
    eng = T.engine()
    obs = T.LevelInputs.fast(hist, gamma, eng) if T.USE_DEVICE_HISTORY else None
    if obs is None:
        isb, isa = T.split_masks(hist, gamma)
        obs = T.LevelInputs(hist, isb, isa, eng, device=T.USE_DEVICE_HISTORY)
    return eng, obs


def _score_device(domain, trials, pool, prior_weight, gamma, lf, want_terms, hist=None):
    """S of every pool row into the pool's device buffer ``S`` (and the
    per-label terms into ``terms``); returns (engine, device pool)."""
    if list(domain.params) != pool.labels:
        raise ValueError("the pool was built for another space (labels differ)")
    eng, obs = _history_inputs(domain, trials, gamma, hist)
    d = pool.device(eng)
    t, lib = eng.torch, eng.lib
    P = len(pool)
    if want_terms and d.terms is None:
        d.terms = t.empty((len(pool.labels), max(P, 1)), dtype=t.float64, device=eng.device)
    if P == 0:
        return eng, d
    sp = ctypes.c_void_p(t.cuda.current_stream(eng.device).cuda_stream)
    todo = [j for j in range(len(pool.labels)) if pool.n_active[j]]
    per = max(1, CHUNK_ELEMS // P)
    init = 1
    for c0 in range(0, max(len(todo), 1), per):
        js = todo[c0:c0 + per]
        off = np.zeros(max(len(js), 1), np.int64)
        d_bl = d_al = None
        if js:
            works = []
            for j in js:
                lab = pool.labels[j]
                w = obs.work(lab, domain.specs[lab], j, n_cand=P, n_total=P)
                w.cand_dev = (j * P, P, d.ranges[j])
                works.append(w)
            res = eng.run(works, prior_weight=prior_weight, lf=lf, precision=64, outputs=True,
                          cand_ptr=d.vals.data_ptr(), device_outputs=True, **obs.run_kwargs)
            off[:] = [r.extra["out_off"] for r in res]
            d_bl, d_al = eng.device_output_ptrs()
        cols = np.asarray(js if js else [0], np.int64)
        _L.check(lib.tpe_pool_fold(d_bl, d_al, off.ctypes.data, cols.ctypes.data, len(js),
                                   d.active.data_ptr(), P, P, init, d.S.data_ptr(),
                                   d.terms.data_ptr() if want_terms else None, P, sp),
                 "tpe_pool_fold")
        init = 0
    if want_terms:  # labels live in no row were not scored: NaN throughout
        for j in range(len(pool.labels)):
            if not pool.n_active[j]:
                d.terms[j].fill_(float("nan"))
    return eng, d


def _topk_device(eng, d, P, k):
    """Rows of the first k untaken rows by d.S, in rank order (numpy int64)."""
    t, lib = eng.torch, eng.lib
    k = min(int(k), P)
    if k <= 0 or P == 0:
        return np.zeros(0, np.int64)
    need = lib.tpe_pool_topk_scratch_bytes(P, k)
    if d.scratch is None or d.scratch.numel() < need:
        d.scratch = t.empty(need, dtype=t.uint8, device=eng.device)
    if d.rows_out is None or d.rows_out.numel() < k:
        d.rows_out = t.empty(k, dtype=t.int64, device=eng.device)
        d.count = t.zeros(1, dtype=t.int64, device=eng.device)
    sp = ctypes.c_void_p(t.cuda.current_stream(eng.device).cuda_stream)
    _L.check(lib.tpe_pool_topk(d.S.data_ptr(), d.taken.data_ptr(), P, k, d.rows_out.data_ptr(),
                               d.count.data_ptr(), d.scratch.data_ptr(), sp), "tpe_pool_topk")
    n = int(d.count.item())
    return d.rows_out[:n].cpu().numpy()


def score_configs(domain, trials, pool, prior_weight=1.0, gamma=0.25, linear_forgetting=25,
                  return_terms=False):
    """S (module doc) of every pool row as an fp64 (P,) array; with
    ``return_terms`` also the (P, L) matrix of per-label terms log l - log g,
    NaN where the label is inactive.  Exact fp64 scoring, whatever the pool
    size.  S[r] is the sequential fp64 sum of row r's terms over its live
    labels in ``domain.params`` order, starting from 0.0."""
    domain = as_domain(domain)
    eng, d = _score_device(domain, trials, pool, prior_weight, gamma, linear_forgetting,
                           return_terms)
    P = len(pool)
    S = d.S[:P].cpu().numpy()
    if not return_terms:
        return S
    return S, np.ascontiguousarray(d.terms[:, :P].cpu().numpy().T)


def startup_rows(pool, seed, k):
    """The startup phase's rows: k of the untaken rows, uniformly without
    replacement, a function of (seed, taken set) alone:
    ``untaken[np.random.RandomState(seed).choice(untaken.size, k, replace=False)]``."""
    untaken = np.flatnonzero(pool.taken == 0)
    k = min(int(k), untaken.size)
    if k == 0:
        return np.zeros(0, np.int64)
    return untaken[np.random.RandomState(seed).choice(untaken.size, k, replace=False)]


def suggest_from_pool(new_ids, domain, trials, seed, pool=None, prior_weight=1.0,
                      n_startup_jobs=20, gamma=0.25, linear_forgetting=25, verbose=True):
    """An ``algo`` for fmin (``partial(tpe.suggest_from_pool, pool=pool)``): one
    document per id, the first id the best untaken row of ``pool`` by
    ``score_configs``, the second the next best, and so on -- larger S first,
    NaN before everything (broadcast_best's argmax), equal scores to the
    smaller row.  The rows are marked taken and entered in ``pool.row_of``.
    Fewer untaken rows than ids: that many documents; none: ``[]`` (fmin then
    stops).  While the history is shorter than ``n_startup_jobs``
    (tpe.py:909-911) the rows are ``startup_rows(pool, seed, k)``.  Under
    torch.distributed every rank scores the whole pool and returns the same
    documents."""
    from . import tpe as T
    if pool is None:
        raise TypeError("suggest_from_pool needs pool= (functools.partial)")
    t0 = time.time()
    domain = as_domain(domain)
    if list(domain.params) != pool.labels:
        raise ValueError("the pool was built for another space (labels differ)")
    k = min(len(new_ids), pool.n_untaken)
    if k == 0:
        return []
    hist = T.collect_history(trials, pool.labels)
    if hist.tids.size < n_startup_jobs:
        rows = startup_rows(pool, seed, k)
    else:
        eng, d = _score_device(domain, trials, pool, prior_weight, gamma, linear_forgetting,
                               False, hist=hist)
        rows = _topk_device(eng, d, len(pool), k)
    rows = [int(r) for r in rows]
    pool.mark_taken(rows)
    ids = list(new_ids)[:len(rows)]
    for tid, r in zip(ids, rows):
        pool.row_of[tid] = r
    docs = trial_docs(ids, domain, trials, [pool.config(r) for r in rows])
    if verbose:
        logger.info("tpe.suggest_from_pool: %d rows in %f seconds" % (len(rows), time.time() - t0))
    return docs
