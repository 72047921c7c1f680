"""Golden vectors of anneal.suggest / mix.suggest from the REFERENCE hyperopt.

Run in the build container only (like make_golden.py, whose reference loader,
stable-argsort patch and writer it uses):

    python tests/golden/make_anneal_golden.py

Writes data only -- histories, the reference's suggestions and picks:

  anneal_single.npz  eleven single-label spaces (one per prior kind), a
                     40-trial history with tied, failed and negative losses,
                     64 new ids x two parameter sets, under a stable argsort:
                     the reference's value and first picked tid per id.
  anneal_flat.npz    the eleven labels in one flat space, 60 trials, 2000 new
                     ids: the first picked tid and the eleven values per call.
  anneal_nested.npz  spaces.nested, 80 trials, 2000 new ids: the root value,
                     the live labels (bitmask) and the number of picks.
  mix_choices.npz    mix.suggest for seeds 0..255, p = (0.1, 0.2, 0.7): the
                     chosen algorithm and the seed handed to it.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import anneal_spaces as AS  # noqa: E402
import spaces as SPACES  # noqa: E402
from make_golden import load_reference, save, stable_argsort  # noqa: E402

SEED = 123
PSETS = [dict(avg_best_idx=2.0, shrink_coef=0.1), dict(avg_best_idx=8.0, shrink_coef=0.5)]


def history(ho, space, n, seed, losses):
    """Trials with n finished documents: values from the reference's
    rand.suggest, losses as given (NaN: a failed trial, no loss)."""
    domain = ho.base.Domain(lambda x: x, space)
    trials = ho.Trials()
    docs = ho.rand.suggest(list(range(n)), domain, trials, seed)
    for doc, loss in zip(docs, losses):
        doc["state"] = ho.base.JOB_STATE_DONE
        doc["result"] = {"status": "fail"} if np.isnan(loss) else \
            {"status": "ok", "loss": float(loss)}
    trials.insert_trial_docs(docs)
    trials.refresh()
    return domain, trials


def columns(trials, labels):
    vals = np.full((len(trials.trials), len(labels)), np.nan)
    for r, doc in enumerate(trials.trials):
        for j, lab in enumerate(labels):
            vv = doc["misc"]["vals"][lab]
            if len(vv):
                vals[r, j] = float(vv[0])
    return vals


def anneal_once(ho, domain, trials, new_id, **kw):
    algo = ho.anneal.AnnealingAlgo(domain, trials, SEED, **kw)
    (doc,) = algo(new_id)
    return doc["misc"]["vals"], list(algo.best_tids)


def single_losses():
    rng = np.random.RandomState(7)
    losses = np.round(rng.uniform(0, 10, 40), 3)
    losses[17] = losses[5]     # two exact ties among finite losses
    losses[30] = losses[22]
    losses[3] = -1.25          # one negative loss
    losses[[8, 19, 33]] = np.nan  # three failed trials
    return losses


def gen_single(ho):
    losses = single_losses()
    new_ids = list(range(40, 104))
    arrays = {"losses": losses}
    for kind in AS.KINDS:
        domain, trials = history(ho, AS.single(ho.hp, kind), 40, 31, losses)
        arrays["hist/" + kind] = columns(trials, ["x"])[:, 0]
        for k, kw in enumerate(PSETS):
            vals, tids = [], []
            with stable_argsort():
                for new_id in new_ids:
                    v, best = anneal_once(ho, domain, trials, new_id, **kw)
                    vals.append(float(v["x"][0]))
                    tids.append(best[0])
            arrays["val/%s/%d" % (kind, k)] = np.asarray(vals)
            arrays["tid/%s/%d" % (kind, k)] = np.asarray(tids, np.int64)
    save("anneal_single", arrays, dict(seed=SEED, new_ids=new_ids, psets=PSETS, kinds=AS.KINDS,
                                       numpy=np.__version__))


def gen_flat(ho):
    losses = np.random.RandomState(8).permutation(60) * 0.37 - 5.0  # distinct, finite
    domain, trials = history(ho, AS.flat(ho.hp), 60, 32, losses)
    new_ids = list(range(60, 2060))
    vals = np.zeros((len(new_ids), len(AS.KINDS)))
    tids = np.zeros(len(new_ids), np.int64)
    for i, new_id in enumerate(new_ids):
        v, best = anneal_once(ho, domain, trials, new_id)
        assert len(best) == 1
        tids[i] = best[0]
        vals[i] = [float(v[lab][0]) for lab in AS.KINDS]
    save("anneal_flat", {"losses": losses, "hist": columns(trials, AS.KINDS),
                         "vals": vals, "tids": tids},
         dict(seed=SEED, first_id=60, labels=AS.KINDS, numpy=np.__version__))


def gen_nested(ho):
    losses = np.random.RandomState(9).permutation(80) * 0.21 - 3.0
    domain, trials = history(ho, SPACES.nested(ho.hp), 80, 33, losses)
    labels = sorted(domain.params)
    new_ids = list(range(80, 2080))
    root = np.zeros(len(new_ids), np.int64)
    live = np.zeros(len(new_ids), np.int64)
    n_picks = np.zeros(len(new_ids), np.int64)
    for i, new_id in enumerate(new_ids):
        v, best = anneal_once(ho, domain, trials, new_id)
        root[i] = int(v["root"][0])
        live[i] = sum(1 << j for j, lab in enumerate(labels) if len(v[lab]))
        n_picks[i] = len(best)
    save("anneal_nested", {"losses": losses, "hist": columns(trials, labels), "root": root,
                           "live": live, "n_picks": n_picks},
         dict(seed=SEED, first_id=80, labels=labels, numpy=np.__version__))


def gen_mix(ho):
    import hyperopt.mix
    seeds = list(range(256))
    chosen = np.zeros(len(seeds), np.int64)
    passed = np.zeros(len(seeds), np.int64)

    def stub(k):
        def algo(new_ids, domain, trials, seed):
            return (k, int(seed))
        return algo

    p_suggest = [(0.1, stub(0)), (0.2, stub(1)), (0.7, stub(2))]
    for i, s in enumerate(seeds):
        chosen[i], passed[i] = hyperopt.mix.suggest([0], None, None, s, p_suggest)
    save("mix_choices", {"chosen": chosen, "passed": passed},
         dict(seeds=seeds, p=[0.1, 0.2, 0.7], numpy=np.__version__))


if __name__ == "__main__":
    ho = load_reference()
    import hyperopt.anneal  # noqa: F401
    gen_single(ho)
    gen_flat(ho)
    gen_nested(ho)
    gen_mix(ho)
