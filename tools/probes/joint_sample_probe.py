#!/usr/bin/env python
"""Times a joint-drawn pool against a factorised one on the C3 space (50 labels,
10k-trial history), same process:

  joint       tpe.Pool.sample(joint=True): tpe_joint_prep of both sets from the
              resident history, tpe_joint_sample of the rows from the below set
              (csrc/tpe_joint_sample.hip), tpe_rows_active, tpe_joint_score of
              the rows under each set;
  factorised  tpe.Pool.sample(): every label's posterior stream drawn and
              scored by the exact fp64 scorers, tpe_rows_active, tpe_pool_fold;
  sampler     tpe_joint_sample alone on the prepared below set (device events
              around the one launch): the new kernel's own share of `joint`.

The first two are the public call followed by a device synchronisation (a born
pool brings nothing back to the host).  Host clock, after warm-up calls,
alternating the two; the p50 (min-max) over --reps calls per pool size.

    python tools/probes/joint_sample_probe.py [--log2 12 16] [--reps 7]
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

SEED = 7


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2", type=int, nargs="+", default=[12, 16], help="pool sizes (log2 P)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", help="also write the JSON result here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("joint_sample_probe needs a GPU")
    import bench
    from hyperopt_amd import joint as J
    from hyperopt_amd import pool as pool_mod
    from hyperopt_amd import tpe

    space = bench.c3_space()
    vals, losses = bench.c3_history(space)
    domain, trials = bench.c3_trials(space, vals, losses)
    labels = list(domain.params)
    kw = dict(prior_weight=1.0, gamma=0.25, linear_forgetting=25)
    eng = tpe.engine()
    hist = tpe.collect_history(trials, labels)
    results = []
    for lg in args.log2:
        P = 1 << lg

        def run(joint):
            pool = tpe.Pool.sample(domain, trials, SEED, P, joint=joint, **kw)
            torch.cuda.synchronize()
            return pool

        times = {"joint": [], "factorised": []}
        for rep in range(args.warmup + args.reps):
            for name in times:  # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(name == "joint")
                if rep >= args.warmup:
                    times[name].append(time.perf_counter() - t0)
        # the sampler kernel alone
        fit, = J.fit(eng, domain, hist, pool_mod._seen_rows(eng, hist), kw["gamma"], len(labels),
                     kw["prior_weight"], kw["linear_forgetting"], J.BANDWIDTH, J.CAT_SMOOTHING)
        out = torch.empty((len(labels), P), dtype=torch.float64, device=eng.device)
        kern = []
        for rep in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            J.sample_device(fit, SEED, out, P, len(labels), 0, P)
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                kern.append(1e-3 * e0.elapsed_time(e1))
        times["sampler"] = kern  # (its three small uploads included)
        rec = {"P": P, "labels": len(labels), "joint_labels": len(J.joint_labels(domain)),
               "history": int(losses.size), "n_below": int(fit.sets[0][1]), "reps": args.reps}
        for name, ts in times.items():
            ts = np.sort(ts)
            rec[name + "_p50_ms"] = 1e3 * float(np.median(ts))
            rec[name + "_min_ms"], rec[name + "_max_ms"] = 1e3 * float(ts[0]), 1e3 * float(ts[-1])
        rec["joint_over_factorised_p50"] = rec["joint_p50_ms"] / rec["factorised_p50_ms"]
        results.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
