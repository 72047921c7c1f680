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

``Pool.sample`` is the pool of a free space: row r holds candidate r of every
label's posterior stream, the draws the exact scorers make anyway.  The rows
never leave the device: ``tpe_rows_active`` decides each row's live labels
from its own choices (``Domain.live_program``), the fold and the top-k are the
ones above, and ``tpe_pool_take`` brings back the winners only
(csrc/tpe_sampled.hip).  ``suggest_sampled`` is the ``algo`` around it: k
distinct documents per call on any space.

``distinct_rows`` names, per row, the first row that holds its configuration
-- or the history row that does: an open-addressing table over whole rows
built on the device (csrc/tpe_distinct.hip), against the history already in
HBM.  ``distinct=True`` makes ``suggest_sampled`` / ``suggest_from_pool``
suggest fresh configurations only.

``GridPool`` is the pool of a Cartesian product of per-label axes.  S is
separable over the axes, so the scorers see every axis value once and
``tpe_grid_fold`` (csrc/tpe_grid.hip) decodes the rows and sums the per-value
terms; the device holds the axes, S and the taken mask, 9 bytes per row.

``joint=True`` (``score_configs``, ``suggest_from_pool``, ``suggest_sampled``)
replaces the sum over the always-live labels by one Parzen mixture over whole
configurations, J = log L_below - log L_above (joint.py; csrc/tpe_joint.hip
builds both sets from the resident history and scores the rows); the fold
adds the terms of the labels under a ``switch`` onto J.
``Pool.sample(joint=True)`` / ``suggest_sampled(joint=True, draw="joint")``
also draw the always-live labels of every row from the below set's joint
mixture (csrc/tpe_joint_sample.hip); ``joint="tree"``, accepted wherever
``joint=True`` is, gives the labels under a ``switch`` joint mixtures as well,
one per group of labels that share an activation condition (joint.py
"Groups"; csrc/tpe_joint_tree.hip), so the candidates themselves follow an
interaction between labels.  ``joint="chain"`` (not on a ``GridPool``, not with
``batch="liar"``) conditions each of those groups on the labels live around it
(joint.py "Chains"; csrc/tpe_joint_chain.hip), so a root label interacts with a
branch label; its sampled pools draw the rows of ``"tree"``.

``batch="liar"`` (``suggest_from_pool``, ``suggest_sampled``, ``pick_batch``;
with ``joint=True`` on a ``Pool`` / ``SampledPool``) makes the k rows of one
call see each other: the top-k of one score is replaced by k picks made one
after the other on the device, each joining the above mixture as the pending
trial it is about to become (joint.py "Batches"; csrc/tpe_joint_lie.hip).  The
host still reads back the k rows only, once.
"""
from __future__ import annotations

import logging
import math
import time

import numpy as np

from . import _lib as _L
from . import joint as _J
from .base import as_domain
from .engine import CONTINUOUS, _params
from .walk import INT_KINDS, int_offset, trial_docs

logger = logging.getLogger(__name__)

# log-densities kept on the device per engine run: a chunk holds as many labels
# as fit (at least one), so the scratch is 2 x 8 x max(P, CHUNK_ELEMS) bytes
CHUNK_ELEMS = 1 << 24


def _same_space(domain, pool):
    if list(domain.params) != pool.labels:
        raise ValueError("the pool was built for another space (labels differ)")


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


def _first_invalid(spec, v, a):
    """(position, what is wrong) of the first entry of ``v`` live under ``a``
    that is not a stored value of the label -- finite, inside ``_bounds``, whole
    for the integer kinds -- or None."""
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
        return int(np.flatnonzero(bad)[0]), what
    return None


def _validate(domain, labels, vals, active):
    """Raise ValueError naming the row and the label of the first invalid entry:
    every live value finite and inside its prior's support, and every row's
    label set the one its own choices make live (``domain.reachable``)."""
    P = vals.shape[0]
    for j, lab in enumerate(labels):
        a, v = active[:, j], vals[:, j]
        bad = _first_invalid(domain.specs[lab], v, a)
        if bad is not None:
            r, what = bad
            raise ValueError("pool row %d, label %r: value %r %s" % (r, lab, float(v[r]), what))
    if P == 0:
        return
    sel = _selectors(domain, labels)
    js = [labels.index(lab) for lab in sel]
    keys = np.where(active[:, js], vals[:, js], -np.inf)
    for want, rows in _live_sets(domain, labels, sel, keys):
        diff = active[rows] != want
        if diff.any():
            i, j = np.argwhere(diff)[0]
            raise ValueError("pool row %d, label %r: %s" % (
                int(rows[i]), labels[j],
                "missing, but live under the row's choices" if want[j]
                else "given, but not live under the row's choices"))


def _selectors(domain, labels):
    """The labels that select a ``switch`` branch, of ``labels``."""
    domain.reachable({})
    sel = getattr(domain, "_selector_labels", None)
    return list(labels) if sel is None else [lab for lab in sel if lab in labels]


def _live_sets(domain, labels, sel, keys):
    """(live mask over ``labels``, its rows) per distinct row of ``keys``, the
    (P, len(sel)) stored values of the selectors (-inf: not decided).  The live
    set depends on the values of the switch selectors only: one ``reachable``
    per distinct assignment."""
    P = keys.shape[0]
    if len(sel):
        uniq, inverse = np.unique(keys, axis=0, return_inverse=True)
        inverse = np.asarray(inverse).reshape(-1)
    else:
        uniq, inverse = np.zeros((1, 0)), np.zeros(P, np.int64)
    for u in range(uniq.shape[0]):
        decided = {lab: _switch_value(domain.specs[lab], uniq[u, i])
                   for i, lab in enumerate(sel) if uniq[u, i] != -np.inf}
        live = set(domain.reachable(decided))
        want = np.fromiter((lab in live for lab in labels), bool, len(labels))
        yield want, np.flatnonzero(inverse == u)


def _host_active(domain, labels, sel, sel_vals):
    """(P, L) activity of rows whose selectors ``sel`` hold the stored values
    ``sel_vals`` (P, len(sel)): each row's ``reachable`` set, every selector
    decided."""
    active = np.zeros((sel_vals.shape[0], len(labels)), bool)
    for want, rows in _live_sets(domain, labels, sel, np.asarray(sel_vals, np.float64)):
        active[rows] = want
    return active


def program_csr(domain):
    """``domain.live_program()`` as tpe_rows_active takes it: (label_off int32
    (L + 1,), clause_off int32 (C + 1,), terms COND_TERM_DTYPE (T,)) in
    ``domain.params`` order, or None without a program."""
    prog = domain.live_program()
    if prog is None:
        return None
    index = {lab: j for j, lab in enumerate(domain.params)}
    label_off, clause_off, terms = [0], [0], []
    for lab in domain.params:
        for clause in prog[lab]:
            terms.extend((index[s], int(b)) for s, b in clause)
            clause_off.append(len(terms))
        label_off.append(len(clause_off) - 1)
    t = np.zeros(len(terms), _L.COND_TERM_DTYPE)
    if terms:
        t["col"], t["value"] = np.asarray(terms, np.int64).T
    return np.asarray(label_off, np.int32), np.asarray(clause_off, np.int32), t


def _range_from_extrema(spec, lo, hi, n_live):
    """``_scoring_range`` from tpe_pool_ranges' (min, max) of the live finite
    values (for the log-domain priors: of those > 0; the log is monotone) and
    the number of live rows."""
    if spec.kind not in CONTINUOUS or not n_live:
        return 0.0, 0.0
    P = _params(spec.kind, spec.args)
    if lo > hi:  # no such value
        return P["prior_mu"], P["prior_mu"]
    if P["family"] == _L.LGMM1:
        return float(np.log(lo)), float(np.log(hi))
    return float(lo), float(hi)


def _scoring_range(spec, live):
    """(min, max) of a label's live values in the scoring coordinate (log x for
    the log-domain priors), the range a ``cand_dev`` work names."""
    if spec.kind not in CONTINUOUS or not live.size:
        return 0.0, 0.0
    P = _params(spec.kind, spec.args)
    if P["family"] == _L.LGMM1:
        with np.errstate(all="ignore"):
            live = np.log(live)
    live = live[np.isfinite(live)]
    mu = P["prior_mu"]
    return (float(live.min()), float(live.max())) if live.size else (mu, mu)


class _DevicePool(object):
    """A pool's mirror on one device: values (L, P) fp64 -- label j's column at
    element j * P, randint(low, high) columns offset-free as the scorers take
    them --, activity (L, P) bytes, the taken mask, and per label the
    (min, max) of its live values in the scoring coordinate."""
    __slots__ = ("vals", "active", "taken", "taken_current", "ranges", "S", "terms", "rows_out",
                 "count", "scratch", "first", "mask", "distinct_scratch", "fits", "parts")

    def __init__(self, vals, active, taken, taken_current, ranges, S, terms=None):
        self.vals, self.active, self.ranges, self.S, self.terms = vals, active, ranges, S, terms
        self.taken, self.taken_current = taken, taken_current
        # made when first needed: the top-k's buffers, ``distinct``'s, and what
        # the last joint scoring left (``_joint_device``)
        self.rows_out = self.count = self.scratch = None
        self.first = self.mask = self.distinct_scratch = None
        self.fits = self.parts = None


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

    @classmethod
    def sample(cls, domain, trials, seed, n_rows, prior_weight=1.0, gamma=0.25,
               linear_forgetting=25, keep_terms=False, joint=False, bandwidth=_J.BANDWIDTH,
               cat_smoothing=_J.CAT_SMOOTHING):
        """``tpe.Pool.sample(domain, trials, seed, n_rows, ...)``: the pool whose
        row r holds candidate r of every label's posterior stream (below
        posterior l; key ``label_key(seed, label)``, candidates [0, n_rows)), every
        label drawn for every row.  A row's live labels are those its own choices
        make live, and the pool is born scored: S(r) (module doc) is the fold of
        the draws' own log l - log g, as the exact fp64 scorers leave them.
        Nothing of size rows x labels crosses to the host.  With no observation
        the posterior is the prior mixture; a startup rule is the caller's.

        Rows are distinct as rows: on a purely discrete space two rows can hold
        the same configuration (``tpe.distinct_rows`` names the first row of
        every configuration; ``suggest_sampled(distinct=True)`` suggests only
        those).  A born S and a later ``score_configs`` of the same rows under the
        same history may differ in their last bits: a log-domain label is scored
        at its drawn log coordinate when born, at log(exp(z)) when injected.

        ``joint=True``: the joint labels (``tpe.joint_labels``: live in every
        configuration) of row r are one draw from the below set's joint
        mixture (joint.py, "Drawing"; ``bandwidth``, ``cat_smoothing``), made
        on the device by ``tpe_joint_sample``; a space without such a label
        raises ValueError.  The labels under a ``switch`` are drawn and scored
        as above, with the same keys and values.  The pool is born with the
        joint criterion's S: J of the drawn rows, then the fold of the live
        non-joint labels' own terms onto it -- ``score_configs(joint=True)`` of
        the same pool (bit for bit on a flat space).  ``keep_terms`` leaves NaN
        in the joint labels' columns.

        ``joint="tree"``: every group of labels that share an activation
        condition (``tpe.joint_groups``) is drawn, for all the rows, from that
        group's own below mixture (joint.py, "Groups": the root group with the
        keys and bits of ``joint=True``, every other group under its own
        component key); the activity follows from the drawn selectors, and
        the pool is born with ``score_configs(joint="tree")`` of its rows.
        ``keep_terms`` leaves NaN everywhere: every label is joint.

        ``joint="chain"``: the rows are those of ``joint="tree"``, column for
        column, for the seed -- the draw is a proposal from the groups' own
        mixtures -- and the pool is born with ``score_configs(joint="chain")``
        of them (joint.py, "Chains")."""
        st = _settings(prior_weight, gamma, linear_forgetting, joint, bandwidth, cat_smoothing)
        return _sample(domain, trials, seed, n_rows, st, keep_terms)

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
                ranges.append(_scoring_range(spec, live))
            d = self._device[eng.device] = _DevicePool(
                t.from_numpy(cols).to(eng.device),
                t.from_numpy(np.ascontiguousarray(self.active.T).view(np.uint8)
                             if P else np.zeros((nl, 1), np.uint8)).to(eng.device),
                t.zeros(max(P, 1), dtype=t.uint8, device=eng.device), False, ranges,
                t.empty(max(P, 1), dtype=t.float64, device=eng.device))
        if not d.taken_current:
            d.taken[:len(self)].copy_(t.from_numpy(self.taken))
            d.taken_current = True
        return d


class SampledPool(Pool):
    """The pool ``Pool.sample`` gives: born on the device, scored there
    (``scores()``: the born S, until the pool is scored again), and an
    ordinary ``Pool`` afterwards.  ``vals`` / ``active`` / ``n_active`` are
    read back on first access -- ``config``, ``keep`` and a ``score_configs``
    on another device do that; ``suggest_sampled`` without ``keep`` does not."""

    def __len__(self):
        return self._n_rows

    def _born(self):
        return self._device[self._born_on]

    def _read_back(self):
        if self._host is None:
            d, P = self._born(), self._n_rows
            active = np.ascontiguousarray(d.active[:, :P].cpu().numpy().T).astype(bool)
            vals = np.ascontiguousarray(d.vals[:, :P].cpu().numpy().T)
            for j, lab in enumerate(self.labels):
                off = int_offset(self.domain.specs[lab])
                if off:
                    vals[:, j] += off
            vals[~active] = np.nan
            self._host = (vals, active)
        return self._host

    @property
    def vals(self):
        return self._read_back()[0]

    @property
    def active(self):
        return self._read_back()[1]

    @property
    def n_active(self):
        if self._n_active is None:
            self._n_active = self._d_n_active.cpu().numpy()
        return self._n_active

    def scores(self):
        """S of every row as the device last computed it (fp64 (P,))."""
        return self._born().S[:self._n_rows].cpu().numpy()

    def terms(self):
        """The born per-label terms, (P, L), NaN where the label is not live
        (``Pool.sample(..., keep_terms=True)``)."""
        d = self._born()
        if d.terms is None:
            raise ValueError("the pool was sampled without keep_terms=True")
        return np.ascontiguousarray(d.terms[:, :self._n_rows].cpu().numpy().T)

    def device(self, eng):
        if eng.device != self._born_on:  # another device: the host copy's mirror
            return Pool.device(self, eng)
        d = self._born()
        if d.ranges is None:  # first use as injected candidates: the columns' ranges
            t, L = eng.torch, len(self.labels)
            specs = [self.domain.specs[lab] for lab in self.labels]
            positive = np.asarray([s.kind in CONTINUOUS and
                                   _params(s.kind, s.args)["family"] == _L.LGMM1
                                   for s in specs], np.uint8)
            out = t.empty(2 * max(L, 1), dtype=t.float64, device=eng.device)
            sp = _J.stream_ptr(eng)
            P = self._n_rows
            _L.check(eng.lib.tpe_pool_ranges(d.vals.data_ptr(), d.active.data_ptr(), P, P, L,
                                             positive.ctypes.data, out.data_ptr(), sp),
                     "tpe_pool_ranges")
            ext = out.cpu().numpy()
            with np.errstate(all="ignore"):
                d.ranges = [_range_from_extrema(s, ext[2 * j], ext[2 * j + 1], self.n_active[j])
                            for j, s in enumerate(specs)]
        if not d.taken_current:
            d.taken[:len(self)].copy_(eng.torch.from_numpy(self.taken))
            d.taken_current = True
        return d


def _rows_active(eng, domain, labels, d, P, sp):
    """The born pool's activity and per-label live counts from its own
    selector columns: on the device by the space's program (tpe_rows_active),
    else -- no program, or one over the kernel's limits -- one ``reachable``
    per distinct selector assignment on the host (only the selector columns
    come back, and the mask goes up).  Returns the counts (device int64)."""
    t, L = eng.torch, len(labels)
    n_active = t.zeros(max(L, 1), dtype=t.int64, device=eng.device)
    csr = program_csr(domain)
    if csr is not None:
        label_off, clause_off, terms = csr
        rc = eng.lib.tpe_rows_active(d.vals.data_ptr(), P, P, L, label_off.ctypes.data,
                                     clause_off.ctypes.data, terms.ctypes.data, len(terms),
                                     d.active.data_ptr(), n_active.data_ptr(), sp)
        if rc == 0:
            return n_active
        if rc != _L.E_UNSUPPORTED:
            _L.check(rc, "tpe_rows_active")
    sel = _selectors(domain, labels)
    js = [labels.index(lab) for lab in sel]
    sv = d.vals[js, :P].cpu().numpy().T if js else np.zeros((P, 0))
    for i, lab in enumerate(sel):
        sv[:, i] += int_offset(domain.specs[lab]) or 0
    active = _host_active(domain, labels, sel, sv)
    d.active[:, :P].copy_(t.from_numpy(np.ascontiguousarray(active.T).view(np.uint8)))
    n_active[:L].copy_(t.from_numpy(active.sum(0).astype(np.int64)))
    return n_active


def _sample(domain, trials, seed, n_rows, st, keep_terms, hist=None):
    """``Pool.sample`` under the settings ``st``.  With ``st.joint`` the joint
    labels come from ``tpe_joint_sample`` and S starts from J; with ``st.lie``
    too the mirror keeps the fit and the born parts (log L_below, log L_above,
    unused) as ``_joint_device`` leaves them."""
    from . import tpe as T
    domain = as_domain(domain)
    labels = list(domain.params)
    P, L = int(n_rows), len(labels)
    if P < 0:
        raise ValueError("n_rows=%d" % P)
    joint = st.joint
    jcols = []
    if joint is not None:  # (ValueError on a space without a joint label)
        jcols = _joint_cols(domain, joint)
    if P == 0:
        return Pool.from_arrays(domain, np.zeros((0, L)), np.zeros((0, L), bool))
    if joint is not None and hist is None:
        hist = T.collect_history(trials, labels)
    if joint is not None and len(jcols) == L:
        eng, obs = T.engine(), None  # (a flat space: no label is left to the engine)
    else:
        eng, obs = _history_inputs(domain, trials, st.gamma, hist)
    t, lib = eng.torch, eng.lib
    d = _DevicePool(
        t.empty((max(L, 1), P), dtype=t.float64, device=eng.device),
        t.zeros((max(L, 1), P), dtype=t.uint8, device=eng.device),
        t.zeros(P, dtype=t.uint8, device=eng.device), True, None,
        t.empty(P, dtype=t.float64, device=eng.device),
        t.empty((max(L, 1), P), dtype=t.float64, device=eng.device) if keep_terms else None)
    sp = _J.stream_ptr(eng)
    per = max(1, CHUNK_ELEMS // P)
    xbuf = t.empty(min(per, max(L, 1)) * P, dtype=t.float64, device=eng.device)

    def draw(js):
        """Labels ``js`` drawn and scored: the draws into their columns, the
        log-densities left in the engine's buffers at the returned offsets."""
        works = [obs.work(labels[j], domain.specs[labels[j]], j, n_cand=P, n_total=P,
                          key=T.label_key(seed, labels[j]), cand_base=0) for j in js]
        res = eng.run(works, prior_weight=st.prior_weight, lf=st.lf, precision=64,
                      outputs=True, device_outputs=True, x_ptr=xbuf.data_ptr(), **obs.run_kwargs)
        off = np.asarray([r.extra["out_off"] for r in res], np.int64)
        for j, o in zip(js, off):  # (device to device)
            d.vals[j].copy_(xbuf[int(o):int(o) + P])
        return off

    todo = [j for j in range(L) if j not in jcols]
    chunks = [todo[c0:c0 + per] for c0 in range(0, len(todo), per)]
    n_active = None
    if joint is not None:
        # the joint labels' columns (with the groups: every group's), for all the
        # rows: one draw per row from the below set's mixture
        fits = _fit(eng, domain, hist, L, st)
        # (joint="chain" draws as "tree" does, from the tree fits: a proposal
        # that its own fits then rank)
        _J.sample_tree_device(_fit(eng, domain, hist, L, st, tree=True)
                              if joint["tree"] == "chain" else fits, seed, d.vals, P, L, 0, P)
    if len(chunks) > 1:
        # the fold runs in label order and needs every row's activity: the
        # selectors' columns first (their draws do not depend on the chunking)
        sel = [labels.index(lab) for lab in _selectors(domain, labels)]
        sel = [j for j in sel if j not in jcols]
        for c0 in range(0, len(sel), per):
            draw(sel[c0:c0 + per])
        n_active = _rows_active(eng, domain, labels, d, P, sp)
    init = 1
    if joint is not None:
        if not chunks:
            n_active = _rows_active(eng, domain, labels, d, P, sp)
        # S starts from J of the drawn rows; the fold below adds the other labels
        # (with the groups every label is joint: S is theirs, and nothing is folded)
        if joint["tree"]:
            _J.score_tree_device(fits, d.vals, d.active, P, L, P, d.S)
        else:
            if st.lie is not None:  # (log L_above of the born rows stays, for the batch)
                d.fits, d.parts = fits, _parts(eng, domain, st, P)
            _J.score_device(fits[0], d.vals, P, L, P, d.S, d.parts)
        init = 0
        if keep_terms:  # the joint labels have no term of their own
            for j in jcols:
                d.terms[j].fill_(float("nan"))
    for js in chunks:
        off = draw(js)
        if n_active is None:
            n_active = _rows_active(eng, domain, labels, d, P, sp)
        d_bl, d_al = eng.device_output_ptrs()
        cols = np.asarray(js, np.int64)
        _L.check(lib.tpe_pool_fold(d_bl, d_al, off.ctypes.data, cols.ctypes.data, len(js),
                                   d.active.data_ptr(), P, P, init, d.S.data_ptr(),
                                   d.terms.data_ptr() if keep_terms else None, P, sp),
                 "tpe_pool_fold")
        init = 0
    if not chunks and joint is None:  # a space without labels: S = 0
        n_active = t.zeros(1, dtype=t.int64, device=eng.device)
        _L.check(lib.tpe_pool_fold(None, None, None, None, 0, None, P, P, 1, d.S.data_ptr(), None,
                                   P, sp), "tpe_pool_fold")
    self = SampledPool.__new__(SampledPool)
    self.domain, self.labels = domain, labels
    self._n_rows, self._born_on, self._host = P, eng.device, None
    self._d_n_active, self._n_active = n_active[:L], None
    self.taken = np.zeros(P, np.uint8)
    self.row_of = {}
    self._device = {eng.device: d}
    return self


class _GridBlock(object):
    """One block of a grid pool: the rows [offset, offset + rows) share the
    selector assignment that makes ``cols`` (label indices in ``domain.params``
    order) live.  Label i of the block takes the ``radix[i]`` axis positions
    from ``pos[i]`` on -- a fixed selector has radix 1 and ``pos`` at its
    value -- and is digit i of the row index, the last label fastest."""
    __slots__ = ("offset", "rows", "cols", "pos", "radix")


class _DeviceGrid(object):
    """A grid pool's mirror on one device: the concatenated axes (fp64,
    randint(low, high) values offset-free), the (min, max) of every axis in the
    scoring coordinate, S (8 bytes per row) and the mask ``tpe_pool_topk``
    reads (taken or excluded, one byte per row)."""
    __slots__ = ("axes", "taken", "taken_current", "ranges", "S", "rows_out", "count", "scratch",
                 "parts")


KEEP_CHUNK = 1 << 20   # rows per call of a grid pool's ``keep``
MAX_BLOCKS = 4096      # the size of Domain.reachable's memo


class GridPool(object):
    """The Cartesian product of per-label axes as a pool, without its rows.

        pool = tpe.GridPool(domain, {"tile_m": [16, 32, 64], "unroll": range(1, 9), ...})

    ``axes`` maps every label of ``domain.params`` to its stored values (as in
    a trial's ``misc["vals"]``), pairwise distinct and valid under ``Pool``'s
    rules (ValueError names the label and the position on the axis).  The
    score of a row is separable, S(row) = sum_l T_l[digit_l(row)] with
    T_l = log l - log g of label l's axis values: the exact scorers see the
    sum of the axis lengths, and ``tpe_grid_fold`` (csrc/tpe_grid.hip) decodes
    the rows.  Nothing of size rows x labels is built except by ``to_pool``.

    Rows.  The pool is a sequence of blocks, one per complete assignment of the
    live selector labels, enumerated depth first: the first undecided live
    selector in ``domain.params`` order takes its axis values in axis order,
    until ``domain.reachable`` adds no label.  A block's rows are the product
    of the axes of its live non-selector labels in ``itertools.product`` order
    (``domain.params`` order, last label fastest); a row's number is its
    block's offset plus its index in the block.  A flat space is one block.

    ``keep(cols)``, optional: called once over all rows in chunks of at most
    ``KEEP_CHUNK``, ``cols`` the {label: float64 array} of the chunk's rows
    (NaN where the label is not live); rows whose entry of the returned mask
    is false are excluded -- never suggested, not counted by ``n_untaken``,
    not drawn in the startup phase.  ``exclude(rows)`` does the same for rows
    given by number.  The rest of the surface is ``Pool``'s.

    ``joint=True`` (any truthy value) marks the grid as carrying the plan of
    the joint criterion (``grid_joint_plan``): ``score_configs(..., joint=True
    | "tree")`` and ``suggest_from_pool(pool=grid, joint=...)`` then rank its
    rows from per-axis factor tables (``joint.score_grid_device``, DESIGN
    3.5.7), with the bits of the materialised pool and still 9 bytes per row
    on the device.  A space without a label that is live in every
    configuration raises ValueError here.  Without it those calls raise
    ValueError, as they always have.
    """

    def __init__(self, domain, axes, keep=None, joint=False):
        domain = as_domain(domain)
        labels = list(domain.params)
        for lab in axes:
            if lab not in domain.params:
                raise ValueError("grid axis %r: not a label of the space" % (lab,))
        self.axes, self.axis_off = [], np.zeros(len(labels) + 1, np.int64)
        for j, lab in enumerate(labels):
            if lab not in axes:
                raise ValueError("grid axis %r: missing (every label of the space needs an axis)"
                                 % (lab,))
            try:
                v = np.array(axes[lab], dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("grid axis %r: its values are not numbers" % (lab,)) from None
            if v.ndim != 1 or v.size == 0:
                raise ValueError("grid axis %r: %s" % (
                    lab, "empty" if v.size == 0 else "not one-dimensional"))
            bad = _first_invalid(domain.specs[lab], v, np.ones(v.size, bool))
            if bad is not None:
                raise ValueError("grid axis %r, position %d: value %r %s"
                                 % (lab, bad[0], float(v[bad[0]]), bad[1]))
            order = np.argsort(v, kind="stable")
            same = np.flatnonzero(v[order][1:] == v[order][:-1])
            if same.size:
                i = int(order[same + 1].min())
                raise ValueError("grid axis %r, position %d: value %r is repeated"
                                 % (lab, i, float(v[i])))
            self.axes.append(v)
            self.axis_off[j + 1] = self.axis_off[j] + v.size
        self.domain, self.labels = domain, labels
        self._enumerate()
        self.joint = bool(joint)
        # (False: the joint labels' plan; True: the groups' of joint="tree", made
        # when first asked for -- not every space that has the one has the other)
        self._joint_plans = {False: grid_joint_plan(self, False)} if self.joint else {}
        P = len(self)
        self.taken = np.zeros(P, np.uint8)
        self.excluded = None
        self.row_of = {}
        self._device = {}
        if keep is not None:
            for lo in range(0, P, KEEP_CHUNK):
                hi = min(P, lo + KEEP_CHUNK)
                mask = np.asarray(keep(self._columns(lo, hi)))
                if mask.shape != (hi - lo,):
                    raise ValueError("keep returned shape %s for %d rows" % (mask.shape, hi - lo))
                self.exclude(lo + np.flatnonzero(~mask.astype(bool)))

    def _enumerate(self):
        domain, labels = self.domain, self.labels
        index = {lab: j for j, lab in enumerate(labels)}
        domain.reachable({})
        selectors = set(domain._selector_labels)
        blocks = []

        def expand(decided, where):
            live = domain.reachable(decided)
            for lab in live:  # (domain.params order)
                if lab in selectors and lab not in decided:
                    spec = domain.specs[lab]
                    for i, v in enumerate(self.axes[index[lab]]):
                        expand(dict(decided, **{lab: _switch_value(spec, v)}),
                               dict(where, **{lab: i}))
                    return
            if len(blocks) == MAX_BLOCKS:
                raise ValueError("the selector axes make more than %d blocks" % MAX_BLOCKS)
            b = _GridBlock()
            b.cols = np.asarray([index[lab] for lab in live], np.int64)
            b.pos = np.asarray([where.get(lab, 0) for lab in live], np.int64)
            b.radix = np.asarray([1 if lab in where else self.axes[index[lab]].size
                                  for lab in live], np.int64)
            b.rows = int(np.prod([int(r) for r in b.radix], dtype=object)) if live else 1
            blocks.append(b)

        expand({}, {})
        self.blocks = blocks
        self.block_off = np.zeros(len(blocks) + 1, np.int64)
        total = 0
        for i, b in enumerate(blocks):
            b.offset = total
            total += b.rows
            if total >= 1 << 62:
                raise ValueError("the grid has more than 2^62 rows")
            self.block_off[i + 1] = total
        live_cols = np.zeros(len(labels), bool)
        for b in blocks:
            live_cols[b.cols] = True
        self.scored = np.flatnonzero(live_cols)  # labels live in some block

    def __len__(self):
        return int(self.block_off[-1])

    def joint_plan(self, tree=False):
        """``grid_joint_plan(self, tree)``, made once; ValueError(GRID_JOINT)
        on a grid built without ``joint=True``."""
        if not self.joint:
            raise ValueError(GRID_JOINT)
        tree = bool(tree)
        if tree not in self._joint_plans:
            self._joint_plans[tree] = grid_joint_plan(self, tree)
        return self._joint_plans[tree]

    @property
    def n_untaken(self):
        gone = self.taken if self.excluded is None else self.taken | self.excluded
        return int(len(self) - np.count_nonzero(gone))

    _rows = Pool._rows

    def _stale(self):
        for d in self._device.values():
            d.taken_current = False

    def mark_taken(self, rows):
        """Rows that are no longer to be suggested (e.g. evaluated elsewhere)."""
        self.taken[self._rows(rows)] = 1
        self._stale()

    def release(self, rows):
        """Rows that may be suggested again; their ``row_of`` entries go.  An
        excluded row cannot be released (ValueError)."""
        rows = self._rows(rows)
        if self.excluded is not None and self.excluded[rows].any():
            raise ValueError("grid row %d is excluded: it cannot be released"
                             % int(rows[np.flatnonzero(self.excluded[rows])[0]]))
        self.taken[rows] = 0
        gone = set(rows.tolist())
        for tid in [t for t, r in self.row_of.items() if r in gone]:
            del self.row_of[tid]
        self._stale()

    def exclude(self, rows):
        """Rows that are not part of the search (module doc: ``keep``)."""
        rows = self._rows(rows)
        if rows.size:
            if self.excluded is None:
                self.excluded = np.zeros(len(self), np.uint8)
            self.excluded[rows] = 1
            self._stale()

    def _block_of(self, row):
        return int(np.searchsorted(self.block_off, row, side="right")) - 1

    def config(self, row):
        """Row ``row`` as the {live label: stored value} dict of a trial."""
        row = int(row)
        if not 0 <= row < len(self):
            raise IndexError("pool rows outside [0, %d)" % len(self))
        b = self.blocks[self._block_of(row)]
        idx = row - b.offset
        specs, out = self.domain.specs, {}
        for i in range(len(b.cols) - 1, -1, -1):
            idx, digit = divmod(idx, int(b.radix[i]))
            j = int(b.cols[i])
            v = self.axes[j][int(b.pos[i]) + digit]
            lab = self.labels[j]
            out[lab] = int(round(v)) if specs[lab].kind in INT_KINDS else float(v)
        return {self.labels[j]: out[self.labels[j]] for j in b.cols}

    def _columns(self, lo, hi):
        """{label: float64 (hi - lo,)} of the rows [lo, hi), NaN where dead."""
        cols = {lab: np.full(hi - lo, np.nan) for lab in self.labels}
        for k in range(self._block_of(lo), len(self.blocks)):
            b = self.blocks[k]
            a, z = max(lo, b.offset), min(hi, b.offset + b.rows)
            if a >= z:
                if b.offset >= hi:
                    break
                continue
            idx = np.arange(a - b.offset, z - b.offset, dtype=np.int64)
            for i in range(len(b.cols) - 1, -1, -1):
                idx, digit = np.divmod(idx, b.radix[i])
                j = int(b.cols[i])
                cols[self.labels[j]][a - lo:z - lo] = self.axes[j][b.pos[i] + digit]
        return cols

    def to_pool(self):
        """The same rows in the same order as a plain ``Pool`` (the (P, L)
        matrix this class avoids: for tests and small grids)."""
        P = len(self)
        vals = np.full((P, len(self.labels)), np.nan)
        for lo in range(0, P, KEEP_CHUNK):
            hi = min(P, lo + KEEP_CHUNK)
            cols = self._columns(lo, hi)
            for j, lab in enumerate(self.labels):
                vals[lo:hi, j] = cols[lab]
        return Pool.from_arrays(self.domain, vals, ~np.isnan(vals))

    # -- device mirror ---------------------------------------------------------
    def device(self, eng):
        """The pool's mirror on ``eng``'s device, uploaded once."""
        d = self._device.get(eng.device)
        t = eng.torch
        P = len(self)
        if d is None:
            flat, ranges = [], []
            for lab, v in zip(self.labels, self.axes):
                spec = self.domain.specs[lab]
                c = v - (int_offset(spec) or 0)
                flat.append(c)
                ranges.append(_scoring_range(spec, c))
            d = _DeviceGrid()
            d.axes = t.from_numpy(np.concatenate(flat)).to(eng.device)
            d.ranges = ranges
            d.taken = t.zeros(max(P, 1), dtype=t.uint8, device=eng.device)
            d.taken_current = False
            d.S = t.empty(max(P, 1), dtype=t.float64, device=eng.device)
            d.rows_out = d.count = d.scratch = d.parts = None
            self._device[eng.device] = d
        if not d.taken_current:
            gone = self.taken if self.excluded is None else self.taken | self.excluded
            d.taken[:P].copy_(t.from_numpy(gone))
            d.taken_current = True
        return d


def _grid_run(eng, obs, domain, pool, d, js, st, want_terms):
    """One engine run over the axis values of the labels ``js`` (label
    indices) of a grid pool: (below pointer, above pointer, out_off, terms) --
    the device log-densities (None without a label), per label of the space
    the offset of its axis position 0 in them (-1: not in the run), and with
    ``want_terms`` {label: T_l}, all NaN for a label that was not in the run."""
    out_off = np.full(len(pool.labels), -1, np.int64)
    d_bl = d_al = None
    if len(js):
        works = []
        for j in js:
            lab = pool.labels[j]
            n = pool.axes[j].size
            w = obs.work(lab, domain.specs[lab], int(j), n_cand=n, n_total=n)
            w.cand_dev = (int(pool.axis_off[j]), n, d.ranges[j])
            works.append(w)
        res = eng.run(works, prior_weight=st.prior_weight, lf=st.lf, precision=64, outputs=True,
                      cand_ptr=d.axes.data_ptr(), device_outputs=True, **obs.run_kwargs)
        out_off[js] = [r.extra["out_off"] for r in res]
        d_bl, d_al = eng.device_output_ptrs()
    terms = None
    if want_terms:
        terms = {lab: np.full(pool.axes[j].size, np.nan) for j, lab in enumerate(pool.labels)}
        if len(js):
            n = int(sum(pool.axes[j].size for j in js))
            bl, al = (eng._bufs[k][:8 * n].cpu().numpy().view(np.float64)
                      for k in ("out_bl", "out_al"))
        for j in js:
            o, m = int(out_off[j]), pool.axes[j].size
            with np.errstate(invalid="ignore"):
                terms[pool.labels[j]] = bl[o:o + m] - al[o:o + m]
    return d_bl, d_al, out_off, terms


def _score_grid(domain, trials, pool, st, want_terms, hist=None, want_parts=False):
    """S of every row of a grid pool into its device buffer ``S``: one engine
    run over the axes of the scored labels, one ``tpe_grid_fold`` per block
    (with ``st.joint``: ``_score_grid_joint``).  Returns (engine, device grid,
    {label: T_l} or None)."""
    _same_space(domain, pool)
    _grid_settings(st, pool)
    if st.joint is not None:
        return _score_grid_joint(domain, trials, pool, st, want_terms, hist, want_parts)
    eng, obs = _history_inputs(domain, trials, st.gamma, hist)
    d = pool.device(eng)
    d_bl, d_al, out_off, terms = _grid_run(eng, obs, domain, pool, d, pool.scored, st, want_terms)
    sp = _J.stream_ptr(eng)
    for b in pool.blocks:
        off = np.ascontiguousarray(out_off[b.cols] + b.pos)
        _L.check(eng.lib.tpe_grid_fold(d_bl, d_al, off.ctypes.data, b.radix.ctypes.data,
                                       len(b.cols), 0, b.rows, d.S.data_ptr() + 8 * b.offset, sp),
                 "tpe_grid_fold")
    return eng, d, terms


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


GRID_JOINT = ("the joint criterion is not separable over the axes of a GridPool; build the grid "
              "with GridPool(..., joint=True), which scores it from per-axis factor tables, or "
              "score its rows as a Pool (GridPool.to_pool())")
GRID_CHAIN = ("joint='chain' is not built for a GridPool: a group's factor tables hold its own "
              "axes, and a chain term needs its context's too (joint.py, \"Not built\"); score "
              "its rows as a Pool (GridPool.to_pool())")


def _grid_settings(st, pool):
    """ValueError where the settings ``st`` ask of the grid pool ``pool`` what
    it was not built with (GRID_JOINT) or what no grid is built for
    (GRID_CHAIN); no-op for any other pool."""
    if st.joint is None or not isinstance(pool, GridPool):
        return
    if not pool.joint:
        raise ValueError(GRID_JOINT)
    if st.joint["tree"] == "chain":
        raise ValueError(GRID_CHAIN)


class GridJointPlan(object):
    """How the joint criterion reads a grid pool (``grid_joint_plan``).

    ``groups``: per group the label indices (``domain.params`` positions) its
    mixture covers -- the joint labels alone, or with ``tree`` every group of
    ``joint_groups(domain)``, the root group first.  ``axis_row[g]``: {label
    index: the row of group g's factor table F that holds the label's axis
    position 0}; a group's axes follow one another in label order and
    ``n_frows[g]`` is their total length.  ``blocks``: one ``GridJointBlock``
    per block of the pool."""
    __slots__ = ("groups", "axis_row", "n_frows", "blocks")


class GridJointBlock(object):
    """One block of a ``GridJointPlan``.  ``radix``: the block's radices (its
    ``_GridBlock``'s).  ``live[g]``: group g is live in the block.
    ``joint[g]``: the positions among the block's labels of group g's labels
    (empty where it is not live).  ``frow[g]``: per label of the block the F
    row of its digit 0 -- ``axis_row[g]`` plus the block's ``pos`` -- or -1 for
    a label that is not group g's and only takes part in the decode (None
    where the group is not live)."""
    __slots__ = ("radix", "live", "joint", "frow")


def grid_joint_plan(pool, tree=False):
    """The ``GridJointPlan`` of the grid pool ``pool`` for ``joint=True``, or
    with ``tree`` for ``joint="tree"``.  Plain Python, no device.  ValueError
    as on a ``Pool``: a space without a label live in every configuration, and
    with ``tree`` switches that are not selected by bare choice / randint
    labels."""
    domain = pool.domain
    index = {lab: j for j, lab in enumerate(pool.labels)}
    if tree:
        groups = [grp.labels for grp in _J.joint_groups(domain)]
    else:
        groups = [[m.label for m in _J.label_models(domain)]]
    plan = GridJointPlan()
    plan.groups = [[index[lab] for lab in labs] for labs in groups]
    plan.axis_row, plan.n_frows = [], []
    for cols in plan.groups:
        rows, at = {}, 0
        for j in cols:
            rows[j] = at
            at += int(pool.axes[j].size)
        plan.axis_row.append(rows)
        plan.n_frows.append(at)
    plan.blocks = []
    for b in pool.blocks:
        where = {int(j): i for i, j in enumerate(b.cols)}
        blk = GridJointBlock()
        blk.radix = np.ascontiguousarray(b.radix, np.int64)
        blk.live, blk.joint, blk.frow = [], [], []
        for g, cols in enumerate(plan.groups):
            inside = [j in where for j in cols]
            # a group's labels share their activation: in or out together, and
            # the root group (the labels live everywhere) always in
            assert all(inside) or not any(inside), (g, cols, list(b.cols))
            assert inside[0] or g > 0
            blk.live.append(inside[0])
            if not inside[0]:
                blk.joint.append([])
                blk.frow.append(None)
                continue
            frow = np.full(len(b.cols), -1, np.int64)
            for j in cols:
                frow[where[j]] = plan.axis_row[g][j] + int(b.pos[where[j]])
            blk.joint.append([where[j] for j in cols])
            blk.frow.append(frow)
        plan.blocks.append(blk)
    return plan


def _score_grid_joint(domain, trials, pool, st, want_terms, hist, want_parts):
    """``_score_grid`` for a grid pool built with ``joint=True``, with the bits
    of the materialised pool: the groups' J from per-axis factor tables
    (``joint.score_grid_device``); then, for ``joint=True`` on a space with a
    ``switch``, per block the univariate terms of the block's other labels
    added onto S in ``domain.params`` order (``tpe_grid_fold_onto``; the joint
    labels are decoded and add nothing), from one engine run over the axes of
    those labels alone.  ``want_parts``: the device grid's ``parts`` receives
    what ``_parts`` describes."""
    from . import tpe as T
    tree = st.joint["tree"]
    plan = pool.joint_plan(tree)  # (ValueError: no joint plan, or no groups)
    if hist is None:
        hist = T.collect_history(trials, pool.labels)
    covered = set(j for cols in plan.groups for j in cols)
    rest = [int(j) for j in pool.scored if int(j) not in covered]
    eng, obs = _history_inputs(domain, trials, st.gamma, hist) if rest else (T.engine(), None)
    d = pool.device(eng)
    d.parts = _parts(eng, domain, st, len(pool)) if want_parts else None
    fits = _fit(eng, domain, hist, len(pool.labels), st)
    _J.score_grid_device(fits, pool, plan, d.axes, d.S, d.parts, tree)
    d_bl, d_al, out_off, terms = _grid_run(eng, obs, domain, pool, d, rest, st, want_terms)
    sp = _J.stream_ptr(eng)
    for b in pool.blocks:
        base = out_off[b.cols]
        if not (base >= 0).any():
            continue
        off = np.ascontiguousarray(np.where(base >= 0, base + b.pos, -1))
        _L.check(eng.lib.tpe_grid_fold_onto(d_bl, d_al, off.ctypes.data, b.radix.ctypes.data,
                                            len(b.cols), 0, b.rows,
                                            d.S.data_ptr() + 8 * b.offset, sp),
                 "tpe_grid_fold_onto")
    return eng, d, terms


def _fit(eng, domain, hist, n_cols, st, tree=None):
    """``joint.fit`` of the history under the settings ``st`` (``tree``: in
    place of the settings' own)."""
    return _J.fit(eng, domain, hist, _seen_rows(eng, hist), st.gamma, n_cols, st.prior_weight,
                  st.lf, st.joint["bandwidth"], st.joint["cat_smoothing"],
                  st.joint["tree"] if tree is None else tree)


def _parts(eng, domain, st, P):
    """The device tensor a joint scoring leaves its parts in: (3, P) for log
    L_below, log L_above and J; with ``tree`` (G, P) filled with NaN for the
    J_g (at least one column)."""
    t = eng.torch
    if st.joint["tree"]:
        return t.full((len(_J.joint_groups(domain)), max(P, 1)), float("nan"), dtype=t.float64,
                      device=eng.device)
    return t.empty((3, max(P, 1)), dtype=t.float64, device=eng.device)


def _joint_device(eng, domain, pool, d, st, hist):
    """J (joint.py) of every pool row into ``d.S`` -- with ``tree`` the groups'
    S (``joint.score_tree_device``) -- and its parts into ``d.parts`` where
    that is a tensor (``_parts``).  The mirror keeps the fit in ``d.fits``."""
    P, L, ld = len(pool), len(pool.labels), d.vals.shape[1]
    d.fits = _fit(eng, domain, hist, L, st)
    if st.joint["tree"]:
        _J.score_tree_device(d.fits, d.vals, d.active, ld, L, P, d.S, d.parts)
        return
    _J.score_device(d.fits[0], d.vals, ld, L, P, d.S, d.parts)
    if d.parts is not None:  # (row 2: J itself, before the fold adds to S)
        d.parts[2, :P].copy_(d.S[:P])


def _score_device(domain, trials, pool, st, want_terms, hist=None, want_parts=False):
    """S of every pool row into the pool's device buffer ``S`` (and the
    per-label terms into ``terms``) under the settings ``st``; returns (engine,
    device pool).  With ``st.joint`` S starts from J and the fold adds the
    other labels' terms, and the mirror keeps the fit in ``fits`` and -- with
    ``want_parts``, and for ``batch="liar"`` -- the parts in ``parts``
    (``_parts``); both are None otherwise."""
    if isinstance(pool, GridPool):  # (ValueError(GRID_JOINT) on a grid without the plan)
        return _score_grid(domain, trials, pool, st, False, hist)[:2]
    _same_space(domain, pool)
    joint = st.joint
    if joint is not None:
        from . import tpe as T
        # (ValueError on a space without a joint label)
        jcols = _joint_cols(domain, joint)
        if hist is None:
            hist = T.collect_history(trials, pool.labels)
        rest = [j for j in range(len(pool.labels)) if pool.n_active[j] and j not in jcols]
        # (a flat space has no other label: no observation inputs, no fold)
        eng, obs = _history_inputs(domain, trials, st.gamma, hist) if rest else (T.engine(), None)
    else:
        eng, obs = _history_inputs(domain, trials, st.gamma, hist)
    d = pool.device(eng)
    t, lib = eng.torch, eng.lib
    P = len(pool)
    if want_terms and d.terms is None:
        d.terms = t.empty((len(pool.labels), max(P, 1)), dtype=t.float64, device=eng.device)
    d.fits = d.parts = None
    if joint is not None and (want_parts or st.lie is not None):
        d.parts = _parts(eng, domain, st, P)
    if P == 0:
        return eng, d
    sp = _J.stream_ptr(eng)
    todo = [j for j in range(len(pool.labels)) if pool.n_active[j]]
    per = max(1, CHUNK_ELEMS // P)
    init = 1
    if joint is not None:
        _joint_device(eng, domain, pool, d, st, hist)
        todo, init = rest, 0
        if want_terms:  # the joint labels have no term of their own
            for j in jcols:
                d.terms[j].fill_(float("nan"))
    for c0 in range(0, len(todo) if joint is not None else max(len(todo), 1), per):
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
            res = eng.run(works, prior_weight=st.prior_weight, lf=st.lf, precision=64,
                          outputs=True, cand_ptr=d.vals.data_ptr(), device_outputs=True,
                          **obs.run_kwargs)
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


def _mirror(pool, eng):
    """The pool's device mirror with a current taken mask; a sampled pool's is
    the one it was born with, as it stands (no ranges: nothing is scored)."""
    if isinstance(pool, SampledPool) and eng.device == pool._born_on:
        d = pool._born()
        if not d.taken_current:
            d.taken[:len(pool)].copy_(eng.torch.from_numpy(pool.taken))
            d.taken_current = True
        return d
    return pool.device(eng)


def _seen_rows(eng, hist):
    """The rows of ``hist`` as tpe_pool_distinct's seen list: (keep-alive
    tensors, vals ptr, active ptr, ld, rows ptr or None, T).  The HBM mirror of
    the trials' cache where LevelInputs would gather from it (position t of the
    list is history row t), else one upload of ``hist.vals`` / ``hist.active``."""
    from . import tpe as T
    t = eng.torch
    n = 0 if hist is None else int(hist.tids.size)
    if n == 0:
        return (), None, None, 0, None, 0
    if T.USE_DEVICE_HISTORY and hist.col is not None:
        dh = hist.col.device_history(eng)
        rows = None
        if hist.rows is not None:
            rows = t.from_numpy(np.ascontiguousarray(hist.rows, np.int32)).to(eng.device)
        return ((dh, rows), dh.vals.data_ptr(), dh.active.data_ptr(), dh.ld,
                None if rows is None else rows.data_ptr(), n)
    active = np.asarray(hist.active, bool)
    vals = t.from_numpy(np.ascontiguousarray(np.where(active, hist.vals, 0.0).T)).to(eng.device)
    act = t.from_numpy(np.ascontiguousarray(active.T).view(np.uint8)).to(eng.device)
    return (vals, act), vals.data_ptr(), act.data_ptr(), n, None, n


def _distinct_device(eng, pool, d, hist):
    """tpe_pool_distinct of the pool's mirror ``d`` against the rows of
    ``hist`` (None: no seen set): ``d.first`` (int64) and ``d.mask`` =
    ``d.taken | (first != row)`` on the device."""
    t, lib = eng.torch, eng.lib
    P, L = len(pool), len(pool.labels)
    if d.first is None:
        d.first = t.empty(max(P, 1), dtype=t.int64, device=eng.device)
        d.mask = t.empty(max(P, 1), dtype=t.uint8, device=eng.device)
    if P == 0:
        return
    _alive, sv, sa, sld, srows, n_seen = _seen_rows(eng, hist)
    need = lib.tpe_pool_distinct_scratch_bytes(P, n_seen)
    if d.distinct_scratch is None or d.distinct_scratch.numel() < need:
        d.distinct_scratch = t.empty(need, dtype=t.uint8, device=eng.device)
    # a history holds randint(low, high) with ``low`` included, a pool without
    shift = np.asarray([int_offset(pool.domain.specs[lab]) or 0 for lab in pool.labels],
                       np.float64)
    sp = _J.stream_ptr(eng)
    _L.check(lib.tpe_pool_distinct(d.vals.data_ptr() if L else None,
                                   d.active.data_ptr() if L else None, d.vals.shape[1], P, L,
                                   sv, sa, sld, srows, n_seen,
                                   shift.ctypes.data if shift.any() else None, 64,
                                   d.taken.data_ptr(), d.first.data_ptr(), d.mask.data_ptr(),
                                   d.distinct_scratch.data_ptr(), sp), "tpe_pool_distinct")


GRID_DISTINCT = ("GridPool rows are distinct by construction; exclude evaluated rows with "
                 "GridPool.exclude")


def distinct_rows(pool, trials=None, domain=None):
    """``first`` (int64 (P,)) of a ``Pool`` / ``SampledPool``: two rows hold the
    same configuration iff the same labels are live in them and every live
    value is equal as an fp64 number (-0.0 == +0.0, all NaNs equal).
    ``first[r]`` is the smallest pool row that holds row r's configuration --
    r itself for the first of its class -- or, with ``trials``, ``-1 - t`` when
    the configuration is that of row t of ``collect_history(trials,
    pool.labels)`` (the smallest such t): the rows a suggest conditions on, so
    pending and failed trials are seen too.  A row is fresh iff ``first[r] ==
    r``.  Computed on the device against the resident history
    (csrc/tpe_distinct.hip); only ``first`` comes back."""
    from . import tpe as T
    if isinstance(pool, GridPool):
        raise ValueError(GRID_DISTINCT)
    if domain is not None:
        _same_space(as_domain(domain), pool)
    if len(pool) == 0:
        return np.zeros(0, np.int64)
    eng = T.engine()
    hist = None if trials is None else T.collect_history(trials, pool.labels)
    d = _mirror(pool, eng)
    _distinct_device(eng, pool, d, hist)
    return d.first[:len(pool)].cpu().numpy()


def _topk_device(eng, d, P, k, taken=None):
    """Rows of the first k untaken rows by d.S, in rank order (numpy int64);
    ``taken``: a device mask to read in place of d.taken."""
    t, lib = eng.torch, eng.lib
    taken = d.taken if taken is None else taken
    k = min(int(k), P)
    if k <= 0 or P == 0:
        return np.zeros(0, np.int64)
    need = lib.tpe_pool_topk_scratch_bytes(P, k)
    if d.scratch is None or d.scratch.numel() < need:
        d.scratch = t.empty(need, dtype=t.uint8, device=eng.device)
    if d.rows_out is None or d.rows_out.numel() < k:
        d.rows_out = t.empty(k, dtype=t.int64, device=eng.device)
        d.count = t.zeros(1, dtype=t.int64, device=eng.device)
    sp = _J.stream_ptr(eng)
    _L.check(lib.tpe_pool_topk(d.S.data_ptr(), taken.data_ptr(), P, k, d.rows_out.data_ptr(),
                               d.count.data_ptr(), d.scratch.data_ptr(), sp), "tpe_pool_topk")
    n = int(d.count.item())
    return d.rows_out[:n].cpu().numpy()


def _joint_kw(joint, bandwidth, cat_smoothing):
    """``_Settings.joint``: None, or the criterion's keywords
    (``tree``: True where the string ``"tree"`` was given -- one mixture per
    group of labels, joint.py "Groups" -- and ``"chain"`` where that string
    was: the groups conditioned on their contexts, joint.py "Chains"; any other
    truthy value is ``joint=True``, ``tree`` False)."""
    if isinstance(joint, str) and joint == "tree":
        tree = True
    elif isinstance(joint, str) and joint == "chain":
        tree = "chain"
    elif not joint:
        return None
    else:
        tree = False
    if not bandwidth > 0.0 or not cat_smoothing >= 0.0:
        raise ValueError("bandwidth=%r must be > 0, cat_smoothing=%r >= 0"
                         % (bandwidth, cat_smoothing))
    return dict(bandwidth=float(bandwidth), cat_smoothing=float(cat_smoothing), tree=tree)


def _joint_cols(domain, jkw):
    """The columns the joint criterion of ``jkw`` covers: the joint labels',
    or with ``tree`` every label's (ValueError on a space without a joint
    label, or without the groups ``tree`` needs)."""
    if jkw.get("tree"):
        labels = list(domain.params)
        return [labels.index(lab) for grp in _J.joint_groups(domain) for lab in grp.labels]
    return [m.col for m in _J.label_models(domain)]


BATCH_LIAR = ("batch='liar' is supported with joint=True on a Pool or a SampledPool "
              "(suggest_from_pool, suggest_sampled, pick_batch)")


class _Settings(object):
    """What a scoring and the picks after it run under: ``prior_weight``,
    ``gamma``, ``lf`` (linear forgetting), ``joint`` (``_joint_kw``) and
    ``lie`` (None, or the lie's weight of ``batch="liar"``)."""
    __slots__ = ("prior_weight", "gamma", "lf", "joint", "lie")

    def __init__(self, prior_weight, gamma, lf, joint=None, lie=None):
        self.prior_weight, self.gamma, self.lf, self.joint, self.lie = \
            prior_weight, gamma, lf, joint, lie


def _settings(prior_weight, gamma, lf, joint=False, bandwidth=_J.BANDWIDTH,
              cat_smoothing=_J.CAT_SMOOTHING, batch=None, lie_weight=1.0, pool=None):
    """The ``_Settings`` of a public call's keywords, after the checks:
    ``_joint_kw``'s, then for a ``batch`` ValueError on any string but
    ``"liar"``, on a ``lie_weight`` that is not a finite number > 0, and on
    what the batch is not built for (joint.py, "Not built"; ``pool``: the
    call's pool, where it has one)."""
    st = _Settings(prior_weight, gamma, lf, _joint_kw(joint, bandwidth, cat_smoothing))
    if batch is None:
        return st
    if batch != "liar":
        raise ValueError("batch=%r: None or 'liar'" % (batch,))
    if not lie_weight > 0.0 or not math.isfinite(lie_weight):
        raise ValueError("lie_weight=%r must be a finite number > 0" % (lie_weight,))
    if st.joint is None:
        raise ValueError(BATCH_LIAR + "; the factorised criterion (joint=False) has no such "
                         "update: its bandwidths depend on the sorted neighbours")
    if st.joint["tree"] == "chain":
        raise ValueError(BATCH_LIAR + "; joint='chain' keeps no log L_above per group")
    if st.joint["tree"]:
        raise ValueError(BATCH_LIAR + "; joint='tree' keeps no log L_above per group")
    if isinstance(pool, GridPool):
        raise ValueError(BATCH_LIAR + "; a GridPool has no row values to lie with "
                         "(GridPool.to_pool())")
    st.lie = float(lie_weight)
    return st


def _liar_device(eng, d, P, k, mask, lie_weight, trace=False):
    """``_topk_device`` for ``batch="liar"``: the rows of ``joint.liar_device``
    on d.S, with the fit and the log L_above the scoring left in the mirror
    (``_joint_device``); ``mask``: ``distinct``'s device mask or None.  The rows
    stay in d.rows_out."""
    t = eng.torch
    k = min(int(k), P)
    if d.rows_out is None or d.rows_out.numel() < k + 1:
        # (with its count, as _topk_device allocates the pair: the count here is
        # entry k of the rows, read back with them)
        d.rows_out = t.empty(k + 1, dtype=t.int64, device=eng.device)
        d.count = t.zeros(1, dtype=t.int64, device=eng.device)
    return _J.liar_device(d.fits[0], d.vals, d.vals.shape[1], d.vals.shape[0], P, d.S, d.parts[1],
                          d.taken, mask, k, lie_weight, trace, d.rows_out)


def _pick(eng, pool, d, k, hist, distinct, st, trace=False):
    """The k rows to hand out, by the scores in the mirror ``d``: the first k
    untaken rows by d.S (``_topk_device``), or with ``st.lie`` the liar batch
    (``_liar_device``; ``trace``: its (rows, S_at_pick, S_k)).  ``distinct``:
    fresh rows only (``_distinct_device`` against ``hist``).  The rows stay in
    d.rows_out."""
    if distinct:
        _distinct_device(eng, pool, d, hist)
    mask = d.mask if distinct else None
    if st.lie is None:
        return _topk_device(eng, d, len(pool), k, mask)
    return _liar_device(eng, d, len(pool), k, mask, st.lie, trace)


def pick_batch(domain, trials, pool, k, distinct=False, return_trace=False, lie_weight=1.0,
               prior_weight=1.0, gamma=0.25, linear_forgetting=25, bandwidth=_J.BANDWIDTH,
               cat_smoothing=_J.CAT_SMOOTHING):
    """The rows ``suggest_from_pool(joint=True, batch="liar")`` would hand out
    for k ids past the startup phase, in pick order (numpy int64; joint.py,
    "Batches"), without marking anything taken.  ``return_trace``: (rows,
    S_at_pick, S_k) -- the score each row was picked at and every row's score
    after the last pick.  A ``GridPool`` raises ValueError."""
    from . import tpe as T
    domain = as_domain(domain)
    st = _settings(prior_weight, gamma, linear_forgetting, True, bandwidth, cat_smoothing, "liar",
                   lie_weight, pool)
    _same_space(domain, pool)
    hist = T.collect_history(trials, pool.labels)
    eng, d = _score_device(domain, trials, pool, st, False, hist=hist)
    if len(pool) == 0:
        none = np.zeros(0, np.int64)
        return (none, np.zeros(0), np.zeros(0)) if return_trace else none
    return _pick(eng, pool, d, k, hist, distinct, st, return_trace)


def score_configs(domain, trials, pool, prior_weight=1.0, gamma=0.25, linear_forgetting=25,
                  return_terms=False, joint=False, bandwidth=_J.BANDWIDTH,
                  cat_smoothing=_J.CAT_SMOOTHING):
    """S (module doc) of every pool row as an fp64 (P,) array; with
    ``return_terms`` also the (P, L) matrix of per-label terms log l - log g,
    NaN where the label is inactive.  Exact fp64 scoring, whatever the pool
    size.  S[r] is the sequential fp64 sum of row r's terms over its live
    labels in ``domain.params`` order, starting from 0.0.

    For a ``GridPool`` the terms are per axis value, not per row:
    ``return_terms`` gives {label: (V_l,) array of T_l}, all NaN for a label
    live in no block.

    ``joint=True``: the joint criterion of ``hyperopt_amd.joint`` -- one
    Parzen mixture over all the labels live in every configuration, J = log
    L_below - log L_above, with ``bandwidth`` and ``cat_smoothing`` -- in
    place of those labels' terms: S[r] starts from J[r] and the terms of the
    row's other live labels (those under a ``switch``) are added in
    ``domain.params`` order; on a flat space S = J.  ``return_terms`` then
    gives (S, terms, J), ``terms`` NaN in the joint labels' columns.  A space
    without a joint label raises ValueError.  A ``GridPool`` built with
    ``joint=True`` is scored from per-axis factor tables, every row with the
    bits of ``GridPool.to_pool()`` (``terms`` is the grid's per-axis dict, all
    NaN for the labels the joint covers; J is per row, as for a ``Pool``); one
    built without it raises ValueError (J is not separable over axes:
    ``GridPool(..., joint=True)`` or ``GridPool.to_pool()``).

    ``joint="tree"``: one such mixture per group of labels that share an
    activation condition (``tpe.joint_groups``; joint.py, "Groups"), each
    built from the history rows and scored on the pool rows in which its
    group is live.  S[r] starts as J_root[r] and the J_g[r] of the other
    groups live in row r are added in group order; no univariate term is
    added.  On a flat space S has the bits of ``joint=True``.
    ``return_terms`` gives (S, terms, J): ``terms`` all NaN, J the (P, G)
    matrix of J_g, NaN where group g is not live in the row.  A space whose
    switches are not selected by bare choice / randint(n) labels raises
    ValueError.

    ``joint="chain"``: the groups of ``"tree"``, each conditioned on its
    context -- the labels outside it that are live whenever it is
    (``tpe.joint_contexts``; joint.py, "Chains"): group g adds C_g = (log
    L_below - log L_ctx,below) - (log L_above - log L_ctx,above) over one
    mixture of the labels ctx + g, so a root label interacts with a branch
    label.  A group with an empty context adds J_g as under ``"tree"``; on a
    flat space S has the bits of ``joint=True``.  ``return_terms`` gives (S,
    terms, C): ``terms`` all NaN, C the (P, G) matrix of J_root and the C_g,
    NaN where group g is not live.  A ``GridPool`` raises ValueError.

    Any other truthy ``joint`` is ``joint=True``."""
    domain = as_domain(domain)
    st = _settings(prior_weight, gamma, linear_forgetting, joint, bandwidth, cat_smoothing)
    grid, tree = isinstance(pool, GridPool), st.joint is not None and st.joint["tree"]
    _grid_settings(st, pool)
    P = len(pool)
    if tree and return_terms:  # (ValueError on a space without the groups, before any other)
        _J.joint_groups(domain)
    if grid:  # (J is read before the fold adds to it: the parts)
        eng, d, terms = _score_grid(domain, trials, pool, st, return_terms,
                                    want_parts=return_terms)
    else:
        eng, d = _score_device(domain, trials, pool, st, return_terms, want_parts=return_terms)
    S = d.S[:P].cpu().numpy()
    if not return_terms:
        return S
    if not grid:
        terms = np.ascontiguousarray(d.terms[:, :P].cpu().numpy().T)
    if st.joint is None:
        return S, terms
    parts, d.parts = d.parts, None
    if tree:
        return S, terms, np.ascontiguousarray(parts[:, :P].cpu().numpy().T)
    return S, terms, parts[2, :P].cpu().numpy()


def startup_rows(pool, seed, k, stale=None):
    """The startup phase's rows: k of the untaken rows (of a grid pool: that are
    not excluded either), uniformly without
    replacement, a function of (seed, taken set) alone:
    ``untaken[np.random.RandomState(seed).choice(untaken.size, k, replace=False)]``.
    ``stale``: a row mask; its rows count as taken (``distinct=True``: the rows
    that are not fresh)."""
    free = pool.taken == 0
    if stale is not None:
        free &= np.asarray(stale) == 0
    if getattr(pool, "excluded", None) is not None:  # (a GridPool's keep / exclude)
        free &= pool.excluded == 0
    untaken = np.flatnonzero(free)
    k = min(int(k), untaken.size)
    if k == 0:
        return np.zeros(0, np.int64)
    return untaken[np.random.RandomState(seed).choice(untaken.size, k, replace=False)]


def suggest_from_pool(new_ids, domain, trials, seed, pool=None, prior_weight=1.0,
                      n_startup_jobs=20, gamma=0.25, linear_forgetting=25, verbose=True,
                      distinct=False, joint=False, bandwidth=_J.BANDWIDTH,
                      cat_smoothing=_J.CAT_SMOOTHING, batch=None, lie_weight=1.0):
    """An ``algo`` for fmin (``partial(tpe.suggest_from_pool, pool=pool)``): one
    document per id, the first id the best untaken row of ``pool`` by
    ``score_configs``, the second the next best, and so on -- larger S first,
    NaN before everything (broadcast_best's argmax), equal scores to the
    smaller row.  The rows are marked taken and entered in ``pool.row_of``.
    Fewer untaken rows than ids: that many documents; none: ``[]`` (fmin then
    stops).  While the history is shorter than ``n_startup_jobs``
    (tpe.py:909-911) the rows are ``startup_rows(pool, seed, k)``.  Under
    torch.distributed every rank scores the whole pool and returns the same
    documents.

    ``distinct=True``: only fresh rows are suggested (``distinct_rows``) -- the
    first row of every configuration of the pool that no row of the history
    holds, pending and failed trials included; a pool with repeated rows never
    gives one configuration twice and never one that ``trials`` already has.
    Fewer fresh untaken rows than ids: that many documents; none: ``[]``.  A
    taken row still counts as the first of its class.  A ``GridPool`` raises
    ValueError: its rows are distinct by construction.

    ``joint=True`` (``joint="tree"``) ranks by ``score_configs(joint=True,
    bandwidth=..., cat_smoothing=...)`` (``joint="tree"``): the same selection,
    ``distinct`` and startup rules, other scores.  A ``GridPool`` needs to
    have been built with ``joint=True`` (else ValueError); its ``keep``,
    ``exclude`` and taken rules are unchanged.  ``joint="chain"`` ranks by
    ``score_configs(joint="chain")`` in the same way; a ``GridPool`` raises
    ValueError.

    ``batch="liar"`` (with ``joint=True`` on a ``Pool`` / ``SampledPool``;
    anything else raises ValueError): the ids' rows are picked one at a time on
    the device, and every pick joins the above mixture with weight
    ``lie_weight`` as the pending trial it is about to become, so the next
    pick keeps away from it (joint.py, "Batches") -- a batch for parallel
    evaluation that does not crowd one mode.  The first document is the one
    ``batch=None`` gives; the startup phase, ``distinct`` and the taken rules
    are unchanged.  ``batch=None``: the k best rows of one score."""
    from . import tpe as T
    if pool is None:
        raise TypeError("suggest_from_pool needs pool= (functools.partial)")
    if distinct and isinstance(pool, GridPool):
        raise ValueError(GRID_DISTINCT)
    st = _settings(prior_weight, gamma, linear_forgetting, joint, bandwidth, cat_smoothing, batch,
                   lie_weight, pool)
    _grid_settings(st, pool)
    t0 = time.time()
    domain = as_domain(domain)
    _same_space(domain, pool)
    k = min(len(new_ids), pool.n_untaken)
    if k == 0:
        return []
    hist = T.collect_history(trials, pool.labels)
    if hist.tids.size < n_startup_jobs:
        stale = None
        if distinct:
            eng = T.engine()
            d = _mirror(pool, eng)
            _distinct_device(eng, pool, d, hist)
            stale = d.first[:len(pool)].cpu().numpy() != np.arange(len(pool))
        rows = startup_rows(pool, seed, k, stale)
    else:
        eng, d = _score_device(domain, trials, pool, st, False, hist=hist)
        rows = _pick(eng, pool, d, k, hist, distinct, st)
    rows = [int(r) for r in rows]
    pool.mark_taken(rows)
    ids = list(new_ids)[:len(rows)]
    for tid, r in zip(ids, rows):
        pool.row_of[tid] = r
    docs = trial_docs(ids, domain, trials, [pool.config(r) for r in rows])
    if verbose:
        logger.info("tpe.suggest_from_pool: %d rows in %f seconds" % (len(rows), time.time() - t0))
    return docs


def _keep_rows(keep, labels, vals, n):
    """Row mask of ``keep`` over n rows, called in chunks of at most
    ``KEEP_CHUNK``; ``vals``: (n, L), NaN where a label is not live."""
    ok = np.ones(n, bool)
    for lo in range(0, n, KEEP_CHUNK):
        hi = min(n, lo + KEEP_CHUNK)
        mask = np.asarray(keep({lab: vals[lo:hi, j] for j, lab in enumerate(labels)}))
        if mask.shape != (hi - lo,):
            raise ValueError("keep returned shape %s for %d rows" % (mask.shape, hi - lo))
        ok[lo:hi] = mask.astype(bool)
    return ok


def _stored_config(domain, labels, vals, active):
    """{live label: stored value} of one row of stored values."""
    out = {}
    for j in np.flatnonzero(active):
        lab = labels[j]
        v = vals[j]
        out[lab] = int(round(v)) if domain.specs[lab].kind in INT_KINDS else float(v)
    return out


def take_rows(pool, rows_dev, k):
    """Rows ``rows_dev[:k]`` (device int64) of a sampled pool as host blocks
    (k, L): stored values (randint's ``low`` restored) and activity --
    tpe_pool_take, the only per-row data such a call reads back."""
    from . import tpe as T
    eng = T.engine()
    d, t, L = pool._born(), eng.torch, len(pool.labels)
    out_v = t.empty((k, max(L, 1)), dtype=t.float64, device=eng.device)
    out_a = t.empty((k, max(L, 1)), dtype=t.uint8, device=eng.device)
    sp = _J.stream_ptr(eng)
    _L.check(eng.lib.tpe_pool_take(d.vals.data_ptr(), d.active.data_ptr(), len(pool), L,
                                   rows_dev.data_ptr(), k, out_v.data_ptr(), out_a.data_ptr(),
                                   sp), "tpe_pool_take")
    vals = out_v.cpu().numpy().reshape(k, max(L, 1))[:, :L]
    active = out_a.cpu().numpy().reshape(k, max(L, 1))[:, :L].astype(bool)
    for j, lab in enumerate(pool.labels):
        off = int_offset(pool.domain.specs[lab])
        if off:
            vals[:, j] += off
    return vals, active


def suggest_sampled(new_ids, domain, trials, seed, n_EI_candidates=4096, keep=None,
                    prior_weight=1.0, n_startup_jobs=20, gamma=0.25, linear_forgetting=25,
                    verbose=True, distinct=False, joint=False, bandwidth=_J.BANDWIDTH,
                    cat_smoothing=_J.CAT_SMOOTHING, draw="factorised", batch=None,
                    lie_weight=1.0):
    """An ``algo`` for fmin on any space: one document per id, k distinct
    points from one history (``max_queue_len=k``, asynchronous backends).

    Past the startup phase it samples a fresh pool of ``n_EI_candidates`` rows
    (``Pool.sample`` with this ``seed``) and returns the first ``len(new_ids)``
    untaken rows by the pool's born S -- larger S first, NaN before
    everything, equal scores to the smaller row.  Only those rows come back
    from the device.  Fewer untaken rows than ids: that many documents; none:
    ``[]``.  While the history is shorter than ``n_startup_jobs`` it returns
    ``rand.suggest_device``'s documents.

    ``keep(cols)``, optional (``GridPool``'s rules): called in chunks of at
    most ``KEEP_CHUNK`` rows with ``cols`` the {label: float64 array} of the
    chunk (NaN where the label is not live); rows whose entry of the returned
    boolean mask is false are marked taken before the selection -- the
    survivors of a feasibility check.  A host predicate costs one readback of
    the pool.  In the startup phase ``keep`` sees ``n_EI_candidates`` prior
    rows (``rand.draw_priors``) and the ids get the first rows it accepts.

    Rows are distinct as rows; on a purely discrete space two of them can hold
    the same configuration, and a fresh pool knows nothing of the trials
    already made.  ``distinct=True`` suggests fresh rows only
    (``distinct_rows``, on the device: no readback): the first row of every
    configuration of the pool that no row of the history holds -- evaluated,
    pending and failed trials alike.  The documents are pairwise distinct
    configurations, none of them in ``trials``; fewer fresh rows than ids:
    that many documents; none: ``[]``, so fmin stops once a discrete space is
    used up.  With ``keep``, a rejected row still counts as the first row of
    its class: a pure predicate gives equal rows equal verdicts.  In the
    startup phase the ``n_EI_candidates`` prior rows go through the same pass
    and the ids get the first fresh (kept) rows in row order.  Under
    torch.distributed every rank samples and scores the same pool and returns
    the same documents.

    ``joint=True``: the pool's rows are ranked by the joint criterion
    (``score_configs(joint=True, ...)``) in place of the factorised S.  Where
    the rows come from is ``draw``'s choice.  ``draw="factorised"`` (the
    default) samples the pool as above -- from the factorised posteriors'
    streams, ``Pool.sample`` unchanged -- and re-ranks it: candidates of the
    factorised l under the joint score.  ``draw="joint"`` (needs
    ``joint=True``; ValueError otherwise, as for any other string) samples it
    with ``Pool.sample(joint=True)``: the always-live labels of every row are
    one draw from the joint l, and the pool is ranked by the S it is born
    with.  ``keep``, ``distinct``, the k-documents rule and the startup phase
    are the same for both.  ``joint="tree"`` is the same with the groups'
    criterion (``score_configs(joint="tree")``) and, under ``draw="joint"``,
    ``Pool.sample(joint="tree")``: the labels under a ``switch`` are drawn
    jointly too.  ``joint="chain"`` ranks by ``score_configs(joint="chain")``
    under either ``draw``; ``draw="joint"`` draws the rows of ``joint="tree"``
    (a draw conditioned on the row's context is not built).

    ``batch="liar"`` (needs ``joint=True``; ValueError otherwise, and for any
    other string): the documents' rows are picked one at a time, each pick
    joining the above mixture with weight ``lie_weight`` (joint.py,
    "Batches"; ``suggest_from_pool``).  log L_above is the one the scoring
    leaves: the pool's born parts under ``draw="joint"``.  ``keep``,
    ``distinct`` and the startup phase are unchanged."""
    from . import rand
    from . import tpe as T
    t0 = time.time()
    if draw not in ("factorised", "joint"):
        raise ValueError("draw=%r: 'factorised' or 'joint'" % (draw,))
    if draw == "joint" and not joint:
        raise ValueError("draw='joint' draws from the joint criterion's below mixture: it needs "
                         "joint=True")
    domain = as_domain(domain)
    st = _settings(prior_weight, gamma, linear_forgetting, joint, bandwidth, cat_smoothing, batch,
                   lie_weight)
    if st.joint is not None:
        _joint_cols(domain, st.joint)  # (ValueError on a space without a joint label)
    labels = list(domain.params)
    n = max(int(n_EI_candidates), 0)
    hist = T.collect_history(trials, labels)
    if hist.tids.size < n_startup_jobs:
        if keep is None and not distinct:
            return rand.suggest_device(new_ids, domain, trials, seed)
        _, draws = rand.draw_priors(domain, seed, n)  # (L, n) stored values
        vals = np.ascontiguousarray(draws.T)
        sel = _selectors(domain, labels)
        active = _host_active(domain, labels, sel, vals[:, [labels.index(s) for s in sel]])
        vals[~active] = np.nan
        ok = np.ones(n, bool) if keep is None else _keep_rows(keep, labels, vals, n)
        if distinct and n:
            eng = T.engine()
            prior = Pool.from_arrays(domain, vals, active)
            d = prior.device(eng)
            _distinct_device(eng, prior, d, hist)
            ok &= d.first[:n].cpu().numpy() == np.arange(n)
        rows = np.flatnonzero(ok)[:len(new_ids)]
        configs = [_stored_config(domain, labels, vals[r], active[r]) for r in rows]
        return trial_docs(list(new_ids)[:len(rows)], domain, trials, configs)
    born = st if draw == "joint" else _Settings(prior_weight, gamma, linear_forgetting)
    pool = _sample(domain, trials, seed, n, born, False, hist=hist)
    if keep is not None and len(pool):
        pool.mark_taken(np.flatnonzero(~_keep_rows(keep, labels, pool.vals, len(pool))))
    k = min(len(new_ids), pool.n_untaken)
    if k == 0:
        return []
    eng = T.engine()
    if st.joint is not None and draw != "joint":  # S: the joint criterion, not the born scores
        _score_device(domain, trials, pool, st, False, hist=hist)
    d = _mirror(pool, eng)
    rows = _pick(eng, pool, d, k, hist, distinct, st)
    if not len(rows):
        return []
    vals, active = take_rows(pool, d.rows_out, len(rows))
    pool.mark_taken(rows)
    configs = [_stored_config(domain, labels, vals[i], active[i]) for i in range(len(rows))]
    docs = trial_docs(list(new_ids)[:len(rows)], domain, trials, configs)
    if verbose:
        logger.info("tpe.suggest_sampled: %d of %d rows in %f seconds"
                    % (len(rows), len(pool), time.time() - t0))
    return docs
