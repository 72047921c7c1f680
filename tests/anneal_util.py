"""Helpers of the annealing tests: trials rebuilt from a fixture's history."""
import numpy as np

from hyperopt_amd import JOB_STATE_DONE, Trials
from hyperopt_amd.base import Domain


def domain_of(space):
    return Domain(lambda p: 0.0, space)


def history_docs(domain, trials, labels, hist, losses, first_tid=0):
    """Finished documents: row r of ``hist`` (NaN: label inactive) with loss
    ``losses[r]`` (NaN: a failed trial without a loss)."""
    ints = {lab for lab in labels if domain.specs[lab].kind in ("randint", "categorical")}
    docs = []
    for r, loss in enumerate(losses):
        tid = first_tid + r
        vals = {lab: [] for lab in domain.params}
        for j, lab in enumerate(labels):
            v = hist[r, j]
            if not np.isnan(v):
                vals[lab] = [int(v) if lab in ints else float(v)]
        misc = dict(tid=tid, cmd=domain.cmd, workdir=domain.workdir, vals=vals,
                    idxs={lab: ([tid] if vals[lab] else []) for lab in vals})
        result = {"status": "fail"} if np.isnan(loss) else {"status": "ok", "loss": float(loss)}
        (doc,) = trials.new_trial_docs([tid], [None], [result], [misc])
        doc["state"] = JOB_STATE_DONE
        docs.append(doc)
    return docs


def make_trials(domain, labels, hist, losses):
    trials = Trials()
    trials.insert_trial_docs(history_docs(domain, trials, labels, np.asarray(hist).reshape(
        len(losses), len(labels)), losses))
    trials.refresh()
    return trials
