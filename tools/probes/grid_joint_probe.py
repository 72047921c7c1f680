#!/usr/bin/env python
"""Times the joint criterion on a grid of P = 2^12 and 2^16 rows of the C3
space (50 labels, all joint; 10k-trial history), same rows, same process:

  grid   tpe.score_configs(GridPool(..., joint=True), joint=True): per set one
         factor table over the axis values (tpe_grid_joint_factors), then
         tpe_grid_joint_score per window of rows (csrc/tpe_grid_joint.hip);
  pool   the same rows materialised (``to_pool()``), the route a grid had
         before: tpe_joint_score of the (P, L) matrix (csrc/tpe_joint.hip).

The grid has two values on ``lg`` labels spread over the label list (every
third label) and one value on the others, so that a tile of rows sees fast
labels, labels of radix 1 between them, and a prefix.  Both routes are the
public call, the host copy of S (8 P bytes) included: it is what synchronises.
They are timed with a host clock, after warm-up calls, alternating the two;
the p50 (min - max) over --reps calls is reported per size, with whether the
scores are equal bit for bit and each route's peak of device memory above what
was allocated before it (the pool's mirror or the grid's included: they are
built inside the first, untimed call).  The per-kernel split wants a run of its
own (--only grid under a kernel trace).

    python tools/probes/grid_joint_probe.py [--log2 12 16] [--reps 7] [--only both]
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


def grid_axes(domain, space, lg, seed=7):
    """Two values on labels 0, 3, 6, ... (lg of them), one on the others."""
    rng = np.random.RandomState(seed)
    kinds = {lab: (kind, a) for lab, kind, a in space}
    axes = {}
    for i, lab in enumerate(domain.params):
        kind, a = kinds[lab]
        m = 2 if i % 3 == 0 and i // 3 < lg else 1
        if kind == "uniform":
            v = rng.uniform(a[0], a[1], m)
        elif kind == "loguniform":
            v = np.exp(rng.uniform(a[0], a[1], m))
        elif kind == "quniform":
            v = a[2] * rng.permutation(int(a[1] / a[2]) + 1)[:m]
        elif kind == "normal":
            v = rng.normal(a[0], a[1], m)
        else:
            v = rng.permutation(a[0])[:m].astype(np.float64)
        axes[lab] = v
    return axes


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2", type=int, nargs="+", default=[12, 16], help="grid sizes (log2 P)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("both", "grid", "pool"), default="both")
    ap.add_argument("--out", help="also write the JSON result here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("grid_joint_probe needs a GPU")
    import bench
    from hyperopt_amd import joint as J
    from hyperopt_amd import tpe

    space = bench.c3_space()
    vals, losses = bench.c3_history(space)
    domain, trials = bench.c3_trials(space, vals, losses)
    results = []
    for lg in args.log2:
        P = 1 << lg
        grid = tpe.GridPool(domain, grid_axes(domain, space, lg), joint=True)
        assert len(grid) == P and len(grid.blocks) == 1
        pool = grid.to_pool() if args.only in ("both", "pool") else None

        def run(p):  # (the copy of S to the host synchronises)
            return tpe.score_configs(domain, trials, p, prior_weight=1.0, gamma=0.25,
                                     linear_forgetting=25, joint=True)

        fns = {"grid": lambda: run(grid), "pool": lambda: run(pool)}
        todo = [n for n in fns if args.only in ("both", n)]
        times = {n: [] for n in todo}
        last, peak = {}, {}
        for rep in range(args.warmup + args.reps):
            for n in todo:  # alternating
                torch.cuda.synchronize()
                if rep == 0:
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                last[n] = fns[n]()
                torch.cuda.synchronize()
                if rep == 0:
                    peak[n] = int(torch.cuda.max_memory_allocated() - before)
                if rep >= args.warmup:
                    times[n].append(time.perf_counter() - t0)
        rec = {"P": P, "labels": len(domain.params), "joint_labels": len(J.joint_labels(domain)),
               "axis_values": int(sum(a.size for a in grid.axes)), "history": int(losses.size),
               "reps": args.reps}
        for n in todo:
            t = np.sort(times[n])
            rec[n + "_p50_ms"] = 1e3 * float(np.median(t))
            rec[n + "_min_ms"], rec[n + "_max_ms"] = 1e3 * float(t[0]), 1e3 * float(t[-1])
            rec[n + "_peak_device_bytes"] = peak[n]
        if len(todo) == 2:
            a, b = last["grid"], last["pool"]
            nan = np.isnan(a)
            rec["same_bits"] = bool(np.array_equal(nan, np.isnan(b)) and
                                    np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64)))
            rec["speedup_p50"] = rec["pool_p50_ms"] / rec["grid_p50_ms"]
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del pool, grid
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    if not all(r.get("same_bits", True) for r in results):
        sys.exit("the two routes give different scores")


if __name__ == "__main__":
    main()
