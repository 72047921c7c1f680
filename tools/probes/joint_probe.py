#!/usr/bin/env python
"""Times the joint criterion against the factorised one on the C3 space (50
labels, 10k-trial history), same pool, same process:

  joint       tpe.score_configs(joint=True): tpe_joint_prep of both sets from
              the resident history, tpe_joint_score of the pool under each
              (csrc/tpe_joint.hip);
  factorised  tpe.score_configs(joint=False): the exact fp64 scorers per label
              and tpe_pool_fold.

Both are the public call, the host copy of S (8 P bytes) included: it is what
synchronises.  They are timed with a host clock, after warm-up calls,
alternating the two; the p50 (min-max) over --reps calls is reported per pool
size, with the overlap of the two top-64 sets.  The per-kernel split wants a
run of its own (--only joint under a kernel trace).

    python tools/probes/joint_probe.py [--log2 12 16] [--reps 7] [--only both]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2", type=int, nargs="+", default=[12, 16], help="pool sizes (log2 P)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("both", "joint", "factorised"), default="both")
    ap.add_argument("--out", help="also write the JSON result here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("joint_probe needs a GPU")
    import bench
    from hyperopt_amd import _lib as L
    from hyperopt_amd import joint as J
    from hyperopt_amd import tpe
    from tools.probes.pool_probe import c3_pool, rank_numpy

    space = bench.c3_space()
    vals, losses = bench.c3_history(space)
    domain, trials = bench.c3_trials(space, vals, losses)
    results = []
    for lg in args.log2:
        P = 1 << lg
        pool = c3_pool(domain, space, P)

        def run(joint):  # (the copy of S to the host synchronises)
            return tpe.score_configs(domain, trials, pool, prior_weight=1.0, gamma=0.25,
                                     linear_forgetting=25, joint=joint)

        fns = {"joint": lambda: run(True), "factorised": lambda: run(False)}
        todo = [n for n in fns if args.only in ("both", n)]
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
        rec = {"P": P, "labels": len(domain.params), "joint_labels": len(J.joint_labels(domain)),
               "history": int(losses.size), "k": K, "reps": args.reps,
               "chunk": int(L.load().tpe_joint_chunk())}
        for n in todo:
            t = np.sort(times[n])
            rec[n + "_p50_ms"] = 1e3 * float(np.median(t))
            rec[n + "_min_ms"], rec[n + "_max_ms"] = 1e3 * float(t[0]), 1e3 * float(t[-1])
        if len(todo) == 2:
            rec["top_k_overlap"] = int(np.intersect1d(rank_numpy(last["joint"], K),
                                                      rank_numpy(last["factorised"], K)).size)
            rec["joint_over_factorised_p50"] = rec["joint_p50_ms"] / rec["factorised_p50_ms"]
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del pool
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
