#!/usr/bin/env python
"""Times the liar batch under the chain criterion (batch="liar-chain",
csrc/tpe_joint_lie.hip) against the plain top-k on the C5 shape: the
``nested`` space (tests/golden/spaces.py), P pool rows and a T-trial history
sampled from its prior with uniform losses, same scored pool, same process,
k = 8.

  topk        pool._topk_device: tpe_pool_topk of the k best rows of the chain S
              and the readback of the rows;
  liar_chain  pool._liar_device(tree="chain"): one tpe_joint_lie_chain_picks (k picks, each a
              lie in every chain fit the pick is live in -- mixture and context
              marginal -- and a new argmax) and the one readback of the rows;
  score       one tpe.score_configs(joint="chain") of the pool; k of them is what
              re-scoring after every pick would cost, for scale;
  score_kept  the same scoring keeping the fits' log L_above and log L_ctx,above
              (``score_tree_device(above=, above_ctx=)``: tpe_joint_chain_rows_keep
              for a fit with a context, one tpe_rows_scatter per window without).

Timing, alternation and the batches' mean pairwise distance are
liar_tree_probe.py's (``spread``).

    python tools/probes/liar_chain_probe.py [--log2 12 16] [--trials 10000] [--reps 7] [--k 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if path not in sys.path:
        sys.path.insert(0, path)


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
        sys.exit("liar_chain_probe needs a GPU")
    from hyperopt_amd import hp, rand, tpe
    from hyperopt_amd import joint as J
    from hyperopt_amd import pool as pool_mod
    from hyperopt_amd.base import Domain
    from liar_tree_probe import spread
    from tests import joint_util as U
    from tests.golden import spaces

    domain = Domain(lambda p: 0.0, spaces.SPACES["nested"](hp))
    rng = np.random.RandomState(1)
    T, k = args.trials, args.k
    trials = U.make_trials(domain, [rand.sample_config(domain, rng) for _ in range(T)],
                           rng.uniform(size=T))
    models = J.label_models(domain, list(domain.params))
    st = pool_mod._settings(1.0, 0.25, 25, "chain", batch="liar-chain")
    plain = pool_mod._settings(1.0, 0.25, 25, "chain")
    results = []
    for lg in args.log2:
        P = 1 << lg
        pool = tpe.Pool(domain, [rand.sample_config(domain, rng) for _ in range(P)])
        hist = tpe.collect_history(trials, pool.labels)
        eng, d = pool_mod._score_device(domain, trials, pool, st, False, hist=hist)
        left = d.fits, d.above, d.above_ctx  # (what the liar-chain scoring left)

        def score(settings):
            pool_mod._score_device(domain, trials, pool, settings, False, hist=hist)
            torch.cuda.synchronize()
            if settings is plain:
                d.fits, d.above, d.above_ctx = left  # (a scoring without the batch clears them)

        fns = {
            "topk": lambda: pool_mod._topk_device(eng, d, P, k),
            "liar_chain": lambda: pool_mod._liar_device(eng, d, P, k, None, st.lie, False, "chain"),
            "score": lambda: score(plain),
            "score_kept": lambda: score(st),
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
            left = d.fits, d.above, d.above_ctx  # (score_kept made new ones: the same values)
        rec = {"P": P, "labels": len(domain.params), "groups": len(d.fits), "history": T, "k": k,
               "reps": args.reps, "n_ctx": [f.n_ctx for f in d.fits],
               "records": sum(len(f.dj.models) for f in d.fits),
               "above_sizes": [f.sets[1][1] for f in d.fits]}
        for n in fns:
            t = np.sort(times[n])
            rec[n + "_p50_ms"] = 1e3 * float(np.median(t))
            rec[n + "_min_ms"], rec[n + "_max_ms"] = 1e3 * float(t[0]), 1e3 * float(t[-1])
        rec["k_scores_p50_ms"] = k * rec["score_p50_ms"]
        for n in ("topk", "liar_chain"):
            rec[n + "_rows"] = [int(r) for r in last[n]]
            rec[n + "_spread"] = spread(models, pool.vals, last[n])
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del pool
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
