#!/usr/bin/env python
"""Times ranking a pool on the C3 space (50 labels, 10k-trial history):

  pool      tpe.score_configs' device path + tpe_pool_topk (k = 64): the pool
            is resident in HBM, only the 64 row indices come back;
  baseline  the route without a pool: one Engine.run per label with the
            label's column as injected host candidates and outputs=True, the
            2 x P x L log-densities read back, numpy sum and stable argsort.

Both are timed with a host clock around calls that end in a device
synchronise, after warm-up calls, alternating the two in one process; the
p50 over --reps calls is reported per pool size, with the largest score
difference and whether both name the same 64 rows.  A kernel trace wants a run
of its own (--only pool under the profiler).

    python tools/probes/pool_probe.py [--log2 16 20] [--reps 7] [--only both]
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

K = 64


def c3_pool(domain, space, P, seed=7):
    """P prior draws of the C3 space as a Pool (domain.params column order)."""
    from hyperopt_amd import tpe
    rng = np.random.RandomState(seed)
    kinds = {lab: (kind, a) for lab, kind, a in space}
    cols = []
    for lab in domain.params:
        kind, a = kinds[lab]
        if kind == "uniform":
            v = rng.uniform(a[0], a[1], P)
        elif kind == "loguniform":
            v = np.exp(rng.uniform(a[0], a[1], P))
        elif kind == "quniform":
            v = np.round(rng.uniform(a[0], a[1], P) / a[2]) * a[2]
        elif kind == "normal":
            v = rng.normal(a[0], a[1], P)
        else:
            v = rng.randint(0, a[0], P).astype(np.float64)
        cols.append(v)
    vals = np.stack(cols, 1)
    return tpe.Pool.from_arrays(domain, vals, np.ones(vals.shape, bool))


def rank_numpy(S, k):
    nan = np.isnan(S)
    idx = np.arange(S.size)
    return idx[np.lexsort((idx, np.where(nan, 0.0, -S), ~nan))][:k]


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 20], help="pool sizes (log2 P)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("both", "pool", "baseline"), default="both")
    ap.add_argument("--out", help="also write the JSON result here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("pool_probe needs a GPU")
    import bench
    from hyperopt_amd import pool as pool_mod
    from hyperopt_amd import tpe

    space = bench.c3_space()
    vals, losses = bench.c3_history(space)
    domain, trials = bench.c3_trials(space, vals, losses)
    labels = list(domain.params)
    kw = dict(prior_weight=1.0, gamma=0.25)
    results = []
    for lg in args.log2:
        P = 1 << lg
        pool = c3_pool(domain, space, P)

        def run_pool():
            st = pool_mod._Settings(kw["prior_weight"], kw["gamma"], 25)
            eng, d = pool_mod._score_device(domain, trials, pool, st, False)
            return pool_mod._topk_device(eng, d, P, K), d  # (the row copy synchronises)

        def run_baseline():
            eng, obs = pool_mod._history_inputs(domain, trials, kw["gamma"])
            S = np.zeros(P)
            for j, lab in enumerate(labels):
                spec = domain.specs[lab]
                w = obs.work(lab, spec, j, n_cand=P, n_total=P)
                w.cand = pool.vals[:, j]  # (no randint(low, high) label in C3: no offset)
                r = eng.run([w], prior_weight=kw["prior_weight"], lf=25, precision=64,
                            outputs=True, **obs.run_kwargs)[0]
                S = S + (r.below_llik - r.above_llik)
            return rank_numpy(S, K), S

        todo = [n for n in ("pool", "baseline") if args.only in ("both", n)]
        fns = {"pool": run_pool, "baseline": run_baseline}
        times = {n: [] for n in todo}
        last = {}
        for rep in range(args.warmup + args.reps):
            for n in todo:  # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[n] = fns[n]()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    times[n].append(time.perf_counter() - t0)
        rec = {"P": P, "labels": len(labels), "history": int(losses.size), "k": K,
               "reps": args.reps}
        for n in todo:
            t = np.sort(times[n])
            rec[n + "_p50_ms"] = 1e3 * float(np.median(t))
            rec[n + "_min_ms"], rec[n + "_max_ms"] = 1e3 * float(t[0]), 1e3 * float(t[-1])
        if len(todo) == 2:
            S_dev = last["pool"][1].S[:P].cpu().numpy()
            rec["max_abs_score_diff"] = float(np.abs(S_dev - last["baseline"][1]).max())
            rec["same_top_k"] = bool(np.array_equal(last["pool"][0], last["baseline"][0]))
            rec["speedup_p50"] = rec["baseline_p50_ms"] / rec["pool_p50_ms"]
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del pool
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
