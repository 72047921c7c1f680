#!/usr/bin/env python
"""Times k = 64 distinct suggestions from a sampled pool on the C3 space (50
labels, 10k-trial history):

  sampled   tpe.Pool.sample (draws, activity and the born S on the device) +
            tpe_pool_topk + tpe_pool_take: only the 64 winners come back;
  baseline  the route without it: the labels' streams read back from
            Engine.run in label chunks (outputs=True; the quantized labels
            through the sampler hook, sample_only=True, since their lattice
            scoring keeps no value per candidate), Pool.from_arrays of the
            rows, then the pool's device scoring + top-k as suggest_from_pool
            runs them.

Both are timed with a host clock around calls that end in a device
synchronise, after warm-up calls, alternating the two in one process; the
p50 (min-max) over --reps calls is reported per pool size, with whether both
name the same 64 rows and the largest |dS| between the born and the re-scored
S.  A kernel trace wants a run of its own (--only sampled under the profiler).

    python tools/probes/sampled_pool_probe.py [--log2 16 20] [--reps 7] [--only both]
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
SEED = 7


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 20], help="pool sizes (log2 P)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("both", "sampled", "baseline"), default="both")
    ap.add_argument("--out", help="also write the JSON result here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("sampled_pool_probe needs a GPU")
    import bench
    from hyperopt_amd import pool as pool_mod
    from hyperopt_amd import tpe

    space = bench.c3_space()
    vals, losses = bench.c3_history(space)
    domain, trials = bench.c3_trials(space, vals, losses)
    labels = list(domain.params)
    results = []
    for lg in args.log2:
        P = 1 << lg

        def run_sampled():
            pool = tpe.Pool.sample(domain, trials, SEED, P)
            eng = tpe.engine()
            d = pool._born()
            rows = pool_mod._topk_device(eng, d, P, K)
            v, a = pool_mod.take_rows(pool, d.rows_out, len(rows))  # (the copy synchronises)
            return rows, v, pool

        def run_baseline():
            eng, obs = pool_mod._history_inputs(domain, trials, 0.25)
            per = max(1, pool_mod.CHUNK_ELEMS // P)
            cols = np.empty((P, len(labels)))
            for c0 in range(0, len(labels), per):
                js = list(range(c0, min(len(labels), c0 + per)))
                works = [obs.work(labels[j], domain.specs[labels[j]], j, n_cand=P, n_total=P,
                                  key=tpe.label_key(SEED, labels[j]), cand_base=0) for j in js]
                for hook, pick in (({"outputs": True}, False), ({"sample_only": True}, True)):
                    part = [(j, w) for j, w in zip(js, works) if w.kind.startswith("q") == pick]
                    if part:
                        res = eng.run([w for _, w in part], prior_weight=1.0, lf=25, precision=64,
                                      **hook, **obs.run_kwargs)
                        for (j, _), r in zip(part, res):
                            cols[:, j] = r.cand
            pool = tpe.Pool.from_arrays(domain, cols, np.ones(cols.shape, bool))
            eng, d = pool_mod._score_device(domain, trials, pool,
                                            pool_mod._Settings(1.0, 0.25, 25), False)
            rows = pool_mod._topk_device(eng, d, P, K)
            return rows, cols[rows], d.S[:P].cpu().numpy()

        todo = [n for n in ("sampled", "baseline") if args.only in ("both", n)]
        fns = {"sampled": run_sampled, "baseline": run_baseline}
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
            S_born = last["sampled"][2].scores()
            rec["max_abs_score_diff"] = float(np.abs(S_born - last["baseline"][2]).max())
            rec["same_top_k"] = bool(np.array_equal(last["sampled"][0], last["baseline"][0]))
            rec["same_values"] = bool(np.array_equal(last["sampled"][1], last["baseline"][1]))
            rec["speedup_p50"] = rec["baseline_p50_ms"] / rec["sampled_p50_ms"]
        results.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
