#!/usr/bin/env python
"""Times the liar batch per group (batch="liar-tree",
csrc/tpe_joint_lie.hip) against the plain top-k on the C5 shape: the
``nested`` space (tests/golden/spaces.py), P pool rows and a T-trial history
sampled from its prior with uniform losses, same scored pool, same process,
k = 8.

  topk        pool._topk_device: tpe_pool_topk of the k best rows of the tree S
              and the readback of the rows;
  liar_tree   pool._liar_device(tree=True): one tpe_joint_lie_chain_picks over fits
              without a context (k picks, each a lie in
              every group the pick is live in, and a new argmax) and the one
              readback of the rows;
  score       one tpe.score_configs(joint="tree") of the pool; k of them is what
              re-scoring after every pick would cost, for scale;
  score_above the same scoring keeping the groups' log L_above
              (``score_tree_device(above=)``: one tpe_rows_scatter per window).

Each is timed with a host clock after warm-up calls, alternating; the p50
(min-max) over --reps calls is reported per pool size.  Both selections read
back their rows, which synchronises; the scorings are followed by a
synchronize.  Also printed: the mean pairwise distance of each batch -- per
label 0 where neither row holds it, 1 where one does or two discrete values
differ, else the difference of the fit coordinates over the prior's sigma,
combined as a Euclidean norm.

    python tools/probes/liar_tree_probe.py [--log2 12 16] [--trials 10000] [--reps 7] [--k 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def spread(models, vals, rows):
    """Mean pairwise distance of the pool rows ``rows`` (module doc)."""
    from hyperopt_amd import _lib as L
    from hyperopt_amd import joint as J
    if len(rows) < 2:
        return 0.0
    total = 0.0
    for m in models:
        x = vals[rows, m.col]
        dead = np.isnan(x)
        if m.kind == L.JOINT_CAT:
            diff = (x[:, None] != x[None, :]).astype(np.float64)
        else:
            t = J._fit(m, np.where(dead, 1.0, x)) / m.sigma
            diff = t[:, None] - t[None, :]
        diff = np.where(dead[:, None] & dead[None, :], 0.0,
                        np.where(dead[:, None] | dead[None, :], 1.0, diff))
        total = total + diff * diff
    return float(np.sqrt(total)[np.triu_indices(len(rows), 1)].mean())


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2", type=int, nargs="+", default=[12, 16], help="pool sizes (log2 P)")
    ap.add_argument("--trials", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--out", help="also write the JSON result here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("liar_tree_probe needs a GPU")
    from hyperopt_amd import hp, rand, tpe
    from hyperopt_amd import joint as J
    from hyperopt_amd import pool as pool_mod
    from hyperopt_amd.base import Domain
    from tests import joint_util as U
    from tests.golden import spaces

    domain = Domain(lambda p: 0.0, spaces.SPACES["nested"](hp))
    rng = np.random.RandomState(1)
    T, k = args.trials, args.k
    trials = U.make_trials(domain, [rand.sample_config(domain, rng) for _ in range(T)],
                           rng.uniform(size=T))
    models = J.label_models(domain, list(domain.params))
    kw = dict(prior_weight=1.0, gamma=0.25, linear_forgetting=25)
    st = pool_mod._settings(1.0, 0.25, 25, "tree", batch="liar-tree")
    plain = pool_mod._settings(1.0, 0.25, 25, "tree")
    results = []
    for lg in args.log2:
        P = 1 << lg
        pool = tpe.Pool(domain, [rand.sample_config(domain, rng) for _ in range(P)])
        hist = tpe.collect_history(trials, pool.labels)
        eng, d = pool_mod._score_device(domain, trials, pool, st, False, hist=hist)
        left = d.fits, d.above  # (what the liar-tree scoring left)

        def score(settings):
            pool_mod._score_device(domain, trials, pool, settings, False, hist=hist)
            torch.cuda.synchronize()
            if settings is plain:
                d.fits, d.above = left  # (a scoring without the batch clears them)
            return None

        fns = {
            "topk": lambda: pool_mod._topk_device(eng, d, P, k),
            "liar_tree": lambda: pool_mod._liar_device(eng, d, P, k, None, st.lie, False, True),
            "score": lambda: score(plain),
            "score_above": lambda: score(st),
        }
        times = {n: [] for n in fns}
        last = {}
        for rep in range(args.warmup + args.reps):
            for n in fns:  # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[n] = fns[n]()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    times[n].append(time.perf_counter() - t0)
            left = d.fits, d.above  # (score_above made new ones: the same values)
        rec = {"P": P, "labels": len(domain.params), "groups": len(d.fits), "history": T, "k": k,
               "reps": args.reps, "above_sizes": [f.sets[1][1] for f in d.fits]}
        for n in fns:
            t = np.sort(times[n])
            rec[n + "_p50_ms"] = 1e3 * float(np.median(t))
            rec[n + "_min_ms"], rec[n + "_max_ms"] = 1e3 * float(t[0]), 1e3 * float(t[-1])
        rec["k_scores_p50_ms"] = k * rec["score_p50_ms"]
        rec["topk_rows"] = [int(r) for r in last["topk"]]
        rec["liar_tree_rows"] = [int(r) for r in last["liar_tree"]]
        rec["topk_spread"] = spread(models, pool.vals, last["topk"])
        rec["liar_tree_spread"] = spread(models, pool.vals, last["liar_tree"])
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del pool
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
