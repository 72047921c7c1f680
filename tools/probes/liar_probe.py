#!/usr/bin/env python
"""Times the liar batch (batch="liar", csrc/tpe_joint_lie.hip) against the plain
top-k on the C3 space (50 labels, 10k-trial history), same scored pool, same
process, k = 8.  Two pools per size: prior draws (``Pool`` + ``score_configs``)
and rows drawn from the joint below mixture (``Pool.sample(joint=True)``, what
``suggest_sampled(draw="joint")`` ranks).

  topk    pool._topk_device: tpe_pool_topk of the k best rows of S_0 and the
          readback of the rows -- what a call without ``batch`` does after scoring;
  liar    pool._liar_device: tpe_joint_lie_picks (k picks, each a lie added to the
          above mixture and a new argmax) and the one readback of the rows;
  score   one tpe.score_configs(joint=True) of the pool; k of them is what
          re-scoring the pool after every pick would cost, for scale.

Each is timed with a host clock after warm-up calls, alternating; the p50
(min-max) over --reps calls is reported per pool size.  Both selections read
back their rows, which synchronises.  Also printed: the mean pairwise distance
of each batch in prior-sigma units -- per continuous or quantized label the
difference of the fit coordinates over the prior's sigma, per discrete label 1
where the options differ, combined as a Euclidean norm.

    python tools/probes/liar_probe.py [--log2 12 16] [--reps 7] [--k 8]
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
    """Mean pairwise distance of the pool rows ``rows`` in prior-sigma units."""
    from hyperopt_amd import _lib as L
    from hyperopt_amd import joint as J
    if len(rows) < 2:
        return 0.0
    cols = []
    for m in models:
        x = vals[rows, m.col]
        if m.kind == L.JOINT_CAT:
            cols.append((x[:, None] != x[None, :]).astype(np.float64))
        else:
            t = J._fit(m, x) / m.sigma
            cols.append(t[:, None] - t[None, :])
    d = np.sqrt(sum(c * c for c in cols))
    return float(d[np.triu_indices(len(rows), 1)].mean())


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2", type=int, nargs="+", default=[12, 16], help="pool sizes (log2 P)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--pools", nargs="+", choices=("prior", "joint"), default=["prior", "joint"],
                    help="where the rows come from: prior draws, or the joint below mixture")
    ap.add_argument("--out", help="also write the JSON result here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("liar_probe needs a GPU")
    import bench
    from hyperopt_amd import joint as J
    from hyperopt_amd import pool as pool_mod
    from hyperopt_amd import tpe
    from tools.probes.pool_probe import c3_pool

    space = bench.c3_space()
    vals, losses = bench.c3_history(space)
    domain, trials = bench.c3_trials(space, vals, losses)
    models = J.label_models(domain)
    kw = dict(prior_weight=1.0, gamma=0.25, linear_forgetting=25)
    st = pool_mod._settings(1.0, 0.25, 25, True, J.BANDWIDTH, J.CAT_SMOOTHING, "liar", 1.0)
    k = args.k
    results = []
    for lg, source in [(lg, s) for lg in args.log2 for s in args.pools]:
        P = 1 << lg
        eng = tpe.engine()
        if source == "prior":  # prior draws, scored
            pool = c3_pool(domain, space, P)
            eng, d = pool_mod._score_device(domain, trials, pool, st, False)
        else:  # rows drawn from the joint below mixture, born scored (draw="joint")
            pool = pool_mod._sample(domain, trials, 7, P, st, False)
            d = pool._born()
        S0 = d.S[:P].cpu().numpy()
        A0 = d.parts[1, :P].cpu().numpy()
        left = d.fits, d.parts  # (what the liar scoring left)

        def score():
            S = tpe.score_configs(domain, trials, pool, joint=True, **kw)
            d.fits, d.parts = left  # (a scoring without the batch clears them)
            return S

        fns = {
            "topk": lambda: pool_mod._topk_device(eng, d, P, k),
            "liar": lambda: pool_mod._liar_device(eng, d, P, k, None, st.lie),
            "score": score,
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
        rec = {"P": P, "pool": source, "labels": len(domain.params),
               "joint_labels": len(models), "history": int(losses.size), "k": k,
               "reps": args.reps, "S0_nan": int(np.isnan(S0).sum()),
               "S0_inf": int(np.isinf(S0).sum()), "A0_finite": int(np.isfinite(A0).sum())}
        for n in fns:
            t = np.sort(times[n])
            rec[n + "_p50_ms"] = 1e3 * float(np.median(t))
            rec[n + "_min_ms"], rec[n + "_max_ms"] = 1e3 * float(t[0]), 1e3 * float(t[-1])
        rec["k_scores_p50_ms"] = k * rec["score_p50_ms"]
        rec["topk_rows"] = [int(r) for r in last["topk"]]
        rec["liar_rows"] = [int(r) for r in last["liar"]]
        rec["topk_spread"] = spread(models, pool.vals, last["topk"])
        rec["liar_spread"] = spread(models, pool.vals, last["liar"])
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del pool
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
