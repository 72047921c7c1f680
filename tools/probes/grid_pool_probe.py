#!/usr/bin/env python
"""Times ranking a Cartesian grid of P = 2^16 and 2^20 rows (five labels, one
of them quantized and one categorical, 10k-trial history), top 64:

  grid      tpe.GridPool: the exact scorers see the sum of the axis lengths
            (80 values at 2^20), tpe_grid_fold writes S, tpe_pool_topk ranks;
  pool      the same rows materialised as a tpe.Pool (``to_pool()``), the
            route a grid had before: every label scored for every row,
            tpe_pool_fold, tpe_pool_topk.

Both are timed with a host clock around calls that end in a device
synchronise, after warm-up calls, alternating the two in one process; the p50
(min - max) over --reps calls is reported per size, with the largest score
difference and whether both name the same 64 rows.  The grid route is also
timed without the top-k (``grid_score``).  A kernel trace wants a run of its
own (--only grid under the profiler).

    python tools/probes/grid_pool_probe.py [--log2 16 20] [--reps 7] [--only both]
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
SPACE = [("u", "uniform", (-5.0, 5.0)), ("lu", "loguniform", (-5.0, 0.0)),
         ("qu", "quniform", (0.0, 100.0, 1.0)), ("n", "normal", (0.0, 2.0)),
         ("c", "randint", (16,))]


def grid_axes(lg):
    """Five axes of 2^lg rows in all, 16 values each at lg = 20."""
    bits = [lg // 5 + (1 if i < lg % 5 else 0) for i in range(5)]
    n = {lab: 1 << b for (lab, _, _), b in zip(SPACE, bits)}
    return {"u": np.linspace(-5.0, 5.0, n["u"]), "lu": np.exp(np.linspace(-4.9, -0.1, n["lu"])),
            "qu": 6.0 * np.arange(n["qu"]), "n": np.linspace(-4.0, 4.0, n["n"]),
            "c": np.arange(n["c"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 20], help="grid sizes (log2 P)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("both", "grid", "pool"), default="both")
    ap.add_argument("--out", help="also write the JSON result here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("grid_pool_probe needs a GPU")
    import bench
    from hyperopt_amd import pool as pool_mod
    from hyperopt_amd import tpe

    vals, losses = bench.c3_history(SPACE)
    domain, trials = bench.c3_trials(SPACE, vals, losses)
    pw, gamma, lf = 1.0, 0.25, 25
    st = pool_mod._Settings(pw, gamma, lf)
    results = []
    for lg in args.log2:
        P = 1 << lg
        grid = tpe.GridPool(domain, grid_axes(lg))
        assert len(grid) == P
        pool = grid.to_pool() if args.only in ("both", "pool") else None

        def run_grid():
            eng, d = pool_mod._score_device(domain, trials, grid, st, False)
            return pool_mod._topk_device(eng, d, P, K), d  # (the row copy synchronises)

        def run_grid_score():
            return pool_mod._score_device(domain, trials, grid, st, False)

        def run_pool():
            eng, d = pool_mod._score_device(domain, trials, pool, st, False)
            return pool_mod._topk_device(eng, d, P, K), d

        fns = {"grid": run_grid, "grid_score": run_grid_score, "pool": run_pool}
        todo = [n for n in fns if args.only == "both" or n.startswith(args.only)]
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
        rec = {"P": P, "axes": [int(a.size) for a in grid.axes], "history": int(losses.size),
               "k": K, "reps": args.reps}
        for n in todo:
            t = np.sort(times[n])
            rec[n + "_p50_ms"] = 1e3 * float(np.median(t))
            rec[n + "_min_ms"], rec[n + "_max_ms"] = 1e3 * float(t[0]), 1e3 * float(t[-1])
        if args.only == "both":
            S_grid = last["grid"][1].S[:P].cpu().numpy()
            S_pool = last["pool"][1].S[:P].cpu().numpy()
            rec["max_abs_score_diff"] = float(np.abs(S_grid - S_pool).max())
            rec["same_top_k"] = bool(np.array_equal(last["grid"][0], last["pool"][0]))
            rec["speedup_p50"] = rec["pool_p50_ms"] / rec["grid_p50_ms"]
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del pool, grid
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    if not all(r.get("same_top_k", True) for r in results):
        sys.exit("the two routes name different rows")


if __name__ == "__main__":
    main()
