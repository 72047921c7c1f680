"""Annealing search (hyperopt/anneal.py:100-391) on the HBM-resident history.

For every live hyperparameter of a new trial the algorithm picks one earlier
trial -- the first of the trials already picked for this new trial that has
the label, else the trial at position ``geometric(1 / avg_best_idx) - 1`` of
the label's trials sorted by loss -- and draws the new value from the label's
prior concentrated around that trial's value; the concentration grows with the
number of observations (``shrink = 1 / (1 + T * shrink_coef)``).

``suggest``: the device path.  The history is the columnar cache's mirror in
HBM (``Columnar.device_history``) with a device loss vector beside it, brought
up to date by uploading only the rows whose loss can have changed.  One
``tpe_anneal_sample`` call per level of the space covers every new trial: a
radix select over the loss bits finds the ranked row without sorting, Philox
draws make the value (csrc/tpe_anneal.hip).  Falls back to ``suggest_host``
when the history is not exactly the cached rows (no cache, a filtered document
list, ``from_tid`` documents, duplicate tids).

``suggest_host``: the same algorithm in numpy, drawing with
``RandomState(seed + new_id)`` in the reference's call order -- on a
single-label space it reproduces the reference's draws.

Two deliberate differences from the reference:
  * streams -- the device path draws with Philox4x32-10 keyed by (seed, label,
    new_id) instead of MT19937 seeded with seed + new_id, so its parity is
    distributional (as rand.suggest_device's);
  * label order -- labels are visited level by level (outer choices first,
    ``Domain.reachable``) and within a level in ``domain.params`` order, where
    the reference follows its pyll graph's evaluation order.  The two agree on
    flat spaces and wherever labels that share a condition are co-active.
Ties between equal losses go to the earlier trial (``np.argsort(kind=
"stable")``; the reference's default sort leaves them unspecified).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import rand
from .base import as_domain, doc_loss
from .walk import (decode, docs_matrix, idxs_vals, next_level, trial_docs, trials_columnar,
                   walk)

_default_avg_best_idx = 2.0
_default_shrink_coef = 0.1

_UNIFORM_KINDS = ("uniform", "quniform", "loguniform", "qloguniform")
_NORMAL_KINDS = ("normal", "qnormal", "lognormal", "qlognormal")


# ---------------------------------------------------------------------------
# history
# ---------------------------------------------------------------------------
def _columnar(domain, trials):
    """(docs, columnar cache or None) of ``trials`` for the domain's labels."""
    return trials_columnar(trials, tuple(domain.params))


def _cache_is_history(docs, col):
    """Whether the cached rows are the history as they stand: every document
    cached, one document per tid in increasing order, no from_tid rows."""
    return col is not None and len(docs) == col.rows and col.keys_increasing \
        and col.n_alias == 0


class _HostHistory(object):
    """Losses and per-label observations in tid order (anneal.py:115-132):
    every document counts, the last document of a tid wins, loss None -> +inf."""

    def __init__(self, domain, docs, col):
        self.labels = list(domain.params)
        if _cache_is_history(docs, col):
            n = col.rows
            self.tids, self.losses = col.key_tid[:n], col.losses()
            self.vals, self.active = col.vals[:n], col.active[:n]
        else:
            by_tid = {}
            for doc in docs:
                by_tid[doc["tid"]] = doc
            tids = sorted(by_tid)
            self.tids = np.asarray(tids, dtype=np.int64)
            self.losses = np.array([doc_loss(by_tid[t]) for t in tids], dtype=np.float64)
            self.vals, self.active = docs_matrix([by_tid[t] for t in tids], self.labels)
        self._rows, self._order = {}, {}

    def rows(self, j):
        """History rows where label j is active, ascending."""
        r = self._rows.get(j)
        if r is None:
            r = self._rows[j] = np.flatnonzero(self.active[:, j])
        return r

    def ranked(self, j):
        """The same rows by ascending loss (stable: NaN last, ties by row)."""
        o = self._order.get(j)
        if o is None:
            rows = self.rows(j)
            o = self._order[j] = rows[np.argsort(self.losses[rows], kind="stable")]
        return o


# ---------------------------------------------------------------------------
# host path
# ---------------------------------------------------------------------------
def _host_draw(spec, val, shrink, rng):
    """One draw of the prior concentrated around ``val`` (anneal.py:225-391),
    with the numpy sampler -- and the operation order -- the reference uses."""
    kind, a = spec.kind, spec.args
    if kind in _UNIFORM_KINDS:
        log_scale = "log" in kind
        low, high = a[0], a[1]
        midpt = np.log(val) if log_scale else val
        half = 0.5 * ((high - low) * shrink)
        midpt = np.clip(midpt, low + half, high - half)
        draw = rng.uniform(midpt - half, midpt + half)
        if log_scale:
            draw = np.exp(draw)
        if kind.startswith("q"):
            draw = np.round(draw / a[2]) * a[2]
        return float(draw)
    if kind in _NORMAL_KINDS:
        mu = val
        if kind == "lognormal":
            mu = np.log(val)
        elif kind == "qlognormal":
            mu = np.log(1e-16 + val)
        draw = rng.normal(mu, a[1] * shrink)
        if "log" in kind:
            draw = np.exp(draw)
        if kind.startswith("q"):
            draw = np.round(draw / a[2]) * a[2]
        return float(draw)
    if kind == "randint":
        low, size = (0, int(a[0])) if a[1] is None else (int(a[0]), int(a[1]) - int(a[0]))
        counts = np.zeros(size)
        counts[int(val) - low] = 1.0
        p = (1 - shrink) * counts + shrink * (1.0 / size)
        return int(np.argmax(rng.multinomial(1, p))) + low
    p = np.asarray(a[0], dtype=np.float64)
    p = p[0] if p.ndim == 2 else p.reshape(-1)
    counts = np.zeros(p.size)
    counts[int(val)] = 1.0
    return int(np.argmax(rng.multinomial(1, (1 - shrink) * counts + shrink * p)))


def _host_config(domain, hist, new_id, seed, avg_best_idx, shrink_coef, trace=None):
    """{label: value} of one new trial, walked level by level."""
    rng = np.random.RandomState(seed + new_id)
    col = {lab: j for j, lab in enumerate(hist.labels)}
    best_rows = []

    def choose(lab):
        spec, j = domain.specs[lab], col[lab]
        T = hist.rows(j).size
        if T == 0:
            return spec.sample(rng)
        row = next((r for r in best_rows if hist.active[r, j]), None)
        if row is None:
            g = rng.geometric(1.0 / avg_best_idx) - 1
            row = int(hist.ranked(j)[int(np.clip(g, 0, T - 1))])
            best_rows.append(row)
        shrink = 1.0 / (1.0 + T * shrink_coef)
        return _host_draw(spec, hist.vals[row, j], shrink, rng)
    config = walk(domain, choose)
    if trace is not None:
        trace.append([int(hist.tids[r]) for r in best_rows])
    return config


def _host_configs(new_ids, domain, trials, seed, avg_best_idx, shrink_coef, trace=None):
    docs, col = _columnar(domain, trials)
    hist = _HostHistory(domain, docs, col)
    return [_host_config(domain, hist, new_id, seed, avg_best_idx, shrink_coef, trace)
            for new_id in new_ids]


def suggest_host(new_ids, domain, trials, seed, avg_best_idx=_default_avg_best_idx,
                 shrink_coef=_default_shrink_coef):
    """anneal.suggest in numpy on the host (no GPU, no library call): one
    document per id, drawn with ``RandomState(seed + new_id)`` in the
    reference's call order (``geometric`` only when a new trial is picked, then
    the value's sampler)."""
    domain = as_domain(domain)
    new_ids = list(new_ids)
    return trial_docs(new_ids, domain, trials,
                      _host_configs(new_ids, domain, trials, seed, avg_best_idx, shrink_coef))


# ---------------------------------------------------------------------------
# device path
# ---------------------------------------------------------------------------
def _records(domain, col, seed, shrink_coef):
    """(tpe_anneal records, prior probability pool) for the domain's labels;
    label j reads history column j."""
    from . import _lib as L
    from .tpe import label_keys_array
    labels, prior, pool = rand._prior_table(domain)
    rec = np.zeros(len(labels), L.ANNEAL_DTYPE)
    for f in ("kind", "n_cat", "a", "b", "q", "p_off"):
        rec[f] = prior[f]
    rec["key"] = label_keys_array(seed, labels)
    rec["col"] = np.arange(len(labels))
    n_active = col.n_active.astype(np.int64)
    rec["n_active"] = n_active
    rec["shrink"] = 1.0 / (1.0 + n_active * float(shrink_coef))
    return labels, rec, pool


def _device_losses(col, dh):
    """The device loss vector beside the device history ``dh`` (one fp64 per
    history row), brought up to date: only the rows at or after the previous
    call's ``Columnar.n_final`` -- the rows whose loss can have changed -- and
    the new rows are uploaded."""
    t = dh.torch
    st = dh.__dict__.get("_anneal_loss")
    if st is None or st["col"] is not col:
        st = dh._anneal_loss = {"col": col, "loss": None, "rows": 0, "final": 0}
    if col.n_final < st["final"]:  # invalidate_loss_cache: every loss is read again
        st["rows"] = st["final"] = 0
    start = min(st["final"], st["rows"])
    losses = col.losses()
    n = col.rows
    if st["loss"] is None or st["loss"].numel() < dh.cap:
        grown = t.empty(dh.cap, dtype=t.float64, device=dh.device)
        if start:
            grown[:start].copy_(st["loss"][:start])
        st["loss"] = grown
    if n > start:
        st["loss"][start:n].copy_(t.from_numpy(losses[start:n]))
    st["rows"], st["final"] = n, col.n_final
    st["uploaded"] = n - start
    return st["loss"]


def sample_level(eng, dh, loss, rec, pool, items, new_ids, avg_best_idx, state, debug=False):
    """One tpe_anneal_sample call: ``items`` (per trial, record indices in
    visiting order) against the device history ``dh`` and loss vector ``loss``.
    ``state``: the chain buffers of ``chain_state``.  Returns the values per
    item (and the debug records with ``debug``)."""
    from . import _lib as L
    t = eng.torch
    n_trials = len(items)
    off = np.zeros(n_trials + 1, np.int32)
    np.cumsum([len(it) for it in items], out=off[1:])
    n_items = int(off[-1])
    if n_items == 0:
        return (np.zeros(0), np.zeros(0, L.ANNEAL_DBG_DTYPE)) if debug else np.zeros(0)
    csr = np.concatenate([off, np.fromiter((j for it in items for j in it), np.int32, n_items)])
    d_csr = t.from_numpy(csr).to(dh.device)
    # values, then the error word: zeroed together, read back together
    d_out = t.zeros(n_items + 1, dtype=t.float64, device=dh.device)
    d_dbg = t.zeros(n_items * L.ANNEAL_DBG_DTYPE.itemsize, dtype=t.uint8, device=dh.device) \
        if debug else None
    stream = t.cuda.current_stream(dh.device).cuda_stream
    L.check(eng.lib.tpe_anneal_sample(
        dh.vals.data_ptr(), dh.active.data_ptr(), dh.ld, dh.n_labels, dh.rows, loss.data_ptr(),
        state["d_rec"], rec.ctypes.data_as(ctypes.c_void_p), len(rec), state["d_pool"],
        d_csr.data_ptr(), d_csr.data_ptr() + 4 * (n_trials + 1), n_items, state["d_ids"],
        n_trials, float(avg_best_idx), state["chain"].data_ptr(), state["d_chain_n"],
        state["chain_ld"], d_out.data_ptr(), d_dbg.data_ptr() if debug else None,
        d_out.data_ptr() + 8 * n_items, ctypes.c_void_p(stream)), "tpe_anneal_sample")
    h_out = d_out.cpu().numpy()
    err = int(h_out[n_items:].view(np.int32)[0])
    if err and not state.get("allow_err"):
        raise L.TpeHipError("tpe_anneal_sample: error flags %d (bit 4: the history's active "
                            "rows differ from the host's counts)" % err)
    state["err"] = state.get("err", 0) | err
    if debug:
        return h_out[:n_items], d_dbg.cpu().numpy().view(L.ANNEAL_DBG_DTYPE)
    return h_out[:n_items]


def chain_state(eng, dh, rec, pool, new_ids):
    """Per-call device inputs in one upload -- the probability pool, the new
    ids, the records and the zeroed chain counts -- and the chain buffer."""
    t = eng.torch
    n = len(new_ids)
    ids = np.asarray(new_ids, dtype=np.int64)
    pool = np.ascontiguousarray(pool, dtype=np.float64)
    parts = [pool.view(np.uint8), ids.view(np.uint8), rec.view(np.uint8).reshape(-1),
             np.zeros(4 * n, np.uint8)]
    d = t.from_numpy(np.concatenate(parts)).to(dh.device)
    base = d.data_ptr()
    o_ids = pool.nbytes
    o_rec = o_ids + ids.nbytes
    o_cn = o_rec + rec.nbytes
    chain_ld = max(len(rec), 1)
    return {"buf": d, "d_pool": base, "d_ids": base + o_ids, "d_rec": base + o_rec,
            "d_chain_n": base + o_cn, "chain_ld": chain_ld,
            "chain": t.empty(max(n * chain_ld, 1), dtype=t.int32, device=dh.device)}


def _device_configs(new_ids, domain, col, seed, avg_best_idx, shrink_coef, trace=None):
    from . import tpe
    eng = tpe.engine()
    dh = col.device_history(eng)
    loss = _device_losses(col, dh)
    labels, rec, pool = _records(domain, col, seed, shrink_coef)
    index = {lab: j for j, lab in enumerate(labels)}
    state = chain_state(eng, dh, rec, pool, new_ids)
    decided_all = [{} for _ in new_ids]
    while True:  # one launch per level covers every trial's next level
        levels = [next_level(domain, decided) for decided in decided_all]
        todo = [level for _, level in levels]
        if not any(todo):
            break
        res = sample_level(eng, dh, loss, rec, pool, [[index[lab] for lab in it] for it in todo],
                           new_ids, avg_best_idx, state, debug=trace is not None)
        vals = res[0] if trace is not None else res
        if trace is not None:
            trace.append((todo, res[1]))
        k = 0
        for decided, it in zip(decided_all, todo):
            for lab in it:
                decided[lab] = decode(domain.specs[lab], vals[k], offset=False)[0]
                k += 1
    return [{lab: decided[lab] for lab in live} for decided, (live, _) in zip(decided_all, levels)]


def _configs(new_ids, domain, trials, seed, avg_best_idx, shrink_coef):
    if not avg_best_idx > 0:
        raise ValueError("avg_best_idx must be positive", avg_best_idx)
    docs, col = _columnar(domain, trials)
    if not _cache_is_history(docs, col):
        return _host_configs(new_ids, domain, trials, seed, avg_best_idx, shrink_coef)
    return _device_configs(new_ids, domain, col, seed, avg_best_idx, shrink_coef)


def suggest(new_ids, domain, trials, seed, avg_best_idx=_default_avg_best_idx,
            shrink_coef=_default_shrink_coef):
    """One document per id in ``new_ids`` (the reference takes exactly one id;
    several are a superset, for ``max_queue_len > 1``).

    avg_best_idx: mean of the geometric distribution over which trial to
        explore around, among the trials sorted by loss (0 is the best).
    shrink_coef: rate at which the sampling neighbourhood shrinks with the
        number of observations."""
    domain = as_domain(domain)
    new_ids = list(new_ids)
    return trial_docs(new_ids, domain, trials,
                      _configs(new_ids, domain, trials, seed, avg_best_idx, shrink_coef))


def suggest_batch(new_ids, domain, trials, seed, avg_best_idx=_default_avg_best_idx,
                  shrink_coef=_default_shrink_coef):
    """(idxs, vals) of the new trials, like rand.suggest_batch, from the same
    per-trial walk as ``suggest``.  The reference's vectorised ``size > 1``
    variant, which draws every trial of the batch without the chain of picked
    trials, is not reproduced: each trial of a batch is annealed on its own."""
    domain = as_domain(domain)
    new_ids = list(new_ids)
    return idxs_vals(new_ids, domain,
                     _configs(new_ids, domain, trials, seed, avg_best_idx, shrink_coef))
