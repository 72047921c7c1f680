"""What tpe, anneal and rand share on the host: the conditional-level walk of a
space, the engine-value -> trial-value rule, the trial-document builders and
the documents -> matrices readers.  No GPU and no library; free functions,
because ``as_domain`` accepts any object with ``specs`` and ``reachable``.
"""
from __future__ import annotations

import numpy as np

from .base import foreign_columnar


# -- the level walk ----------------------------------------------------------
def next_level(domain, decided):
    """One step of the walk: (live labels given the decided {label: value},
    those of them not decided yet -- the next level, empty at the end)."""
    live = domain.reachable(decided)
    return live, [lab for lab in live if lab not in decided]


def walk(domain, choose):
    """The walk to its end, one trial on the host: ``choose(label)`` gives a
    label's value, level by level and within a level in ``domain.params``
    order.  Returns {label: value} of the labels live under those values."""
    decided = {}
    while True:
        live, todo = next_level(domain, decided)
        if not todo:
            return {lab: decided[lab] for lab in live}
        for lab in todo:
            decided[lab] = choose(lab)


# -- engine value -> trial value ---------------------------------------------
INT_KINDS = ("randint", "categorical")


def decode(spec, value, offset=True):
    """Device value -> (value used by switches, value stored in the trial).
    TPE's engine values are offset-free: the stored value of randint(low,
    high) gets ``low`` back (tpe.py:945-948).  ``offset=False``: the value is
    a prior draw, ``low`` included."""
    if spec.kind not in INT_KINDS:
        return float(value), float(value)
    k = int(round(value))
    if offset and spec.kind == "randint" and spec.args[1] is not None:
        return k, k + int(spec.args[0])
    return k, k


def int_offset(spec):
    """None for a continuous label, else what ``decode`` adds to the value."""
    return decode(spec, 0)[1] if spec.kind in INT_KINDS else None


def decode_level(plan, values, switch, stored):
    """``decode`` over a level whose (label, int_offset) ``plan`` is cached."""
    for (lab, off), v in zip(plan, values):
        if off is None:
            switch[lab] = stored[lab] = float(v)
        else:
            switch[lab] = k = int(round(v))
            stored[lab] = k + off


# -- new trial documents -----------------------------------------------------
def misc(domain, new_id, config):
    return dict(tid=new_id, cmd=domain.cmd, workdir=domain.workdir,
                idxs={lab: ([new_id] if lab in config else []) for lab in domain.params},
                vals={lab: ([config[lab]] if lab in config else []) for lab in domain.params})


def trial_docs(new_ids, domain, trials, configs):
    """One new document per id from its {live label: value} config."""
    rval = []
    for new_id, config in zip(new_ids, configs):
        rval.extend(trials.new_trial_docs([new_id], [None], [domain.new_result()],
                                          [misc(domain, new_id, config)]))
    return rval


def idxs_vals(new_ids, domain, configs):
    """The same trials as per-label (ids, values) lists."""
    idxs = {lab: [] for lab in domain.params}
    vals = {lab: [] for lab in domain.params}
    for new_id, config in zip(new_ids, configs):
        for lab, v in config.items():
            idxs[lab].append(new_id)
            vals[lab].append(v)
    return idxs, vals


# -- reading trials ----------------------------------------------------------
def trials_columnar(trials, labels):
    """(docs, columnar cache or None) of ``trials`` for ``labels``."""
    docs = trials.trials
    if hasattr(trials, "columnar"):
        return docs, trials.columnar(labels)
    # the reference's Trials (fmin(algo=hyperopt_amd.tpe.suggest)): a cache beside it
    if not isinstance(docs, list):
        docs = list(docs)
    return docs, foreign_columnar(trials, docs, labels)


def docs_matrix(docs, labels):
    """(vals, active) (len(docs), len(labels)) by the reference's walk over
    every document and label (miscs_to_idxs_vals, base.py:200-214)."""
    index = {lab: j for j, lab in enumerate(labels)}
    vals = np.full((len(docs), len(labels)), np.nan)
    active = np.zeros((len(docs), len(labels)), bool)
    for r, d in enumerate(docs):
        for lab, vv in d["misc"]["vals"].items():
            j = index.get(lab)
            if j is not None and len(vv):
                vals[r, j] = float(vv[0])
                active[r, j] = True
    return vals, active
