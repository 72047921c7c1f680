#!/usr/bin/env python
"""Times the distinct-configuration pass of a sampled pool against the route
without it, on the C3 space (50 labels, 10k-trial history) and on its discrete
labels alone (the 10 quantized and 10 categorical ones; "few": 2 + 2 of them;
"two": 1 + 1, 808 configurations, where classes are large):

  device    tpe_pool_distinct of the pool against the resident history
            (pool._distinct_device): first and the top-k mask stay in HBM;
  host      what a caller would write: read back the pool's values and
            activity, np.unique(return_index=True) over a void view of the
            history rows followed by the pool rows, upload the mask;
  suggest   tpe.suggest_sampled(8 ids) with distinct=True and distinct=False.

Timed with a host clock around calls that end in a device synchronise, after
warm-up calls, the routes alternating in one process (device with host, then
the two suggests, the order within a pair swapped every call); p50 (min-max) over
--reps calls per pool size, with whether both routes give the same mask and
how many rows are fresh.

    python tools/probes/distinct_probe.py [--log2 16 20] [--reps 7] [--out FILE]
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

K = 8
SEED = 7


def _void_rows(vals, active):
    # (-0.0 + 0.0 = +0.0; C3 draws no NaN)
    rows = np.ascontiguousarray(np.where(active, vals, 0.0) + 0.0)
    packed = np.ascontiguousarray(np.concatenate(
        [rows.view(np.uint8).reshape(len(rows), -1), active.astype(np.uint8)], axis=1))
    return packed.view(np.dtype((np.void, packed.shape[1]))).reshape(-1)


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 20], help="pool sizes (log2 P)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spaces", nargs="+", default=["c3", "discrete", "few", "two"],
                    choices=("c3", "discrete", "few", "two"))
    ap.add_argument("--out", help="also write the JSON result here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("distinct_probe needs a GPU")
    import bench
    from hyperopt_amd import pool as pool_mod
    from hyperopt_amd import tpe
    from hyperopt_amd.walk import int_offset

    results = []
    for name in args.spaces:
        space = bench.c3_space()
        if name != "c3":
            space = [s for s in space if s[1] in ("quniform", "randint")]
        if name in ("few", "two"):
            space = space[:4 if name == "few" else 2]
        vals, losses = bench.c3_history(space)
        domain, trials = bench.c3_trials(space, vals, losses)
        labels = list(domain.params)
        hist = tpe.collect_history(trials, labels)
        shift = np.asarray([int_offset(domain.specs[lab]) or 0 for lab in labels], np.float64)
        eng = tpe.engine()
        for lg in args.log2:
            P = 1 << lg
            pool = tpe.Pool.sample(domain, trials, SEED, P)
            d = pool._born()

            def run_device():
                pool_mod._distinct_device(eng, pool, d, hist)
                return d.mask

            def run_host():
                v = d.vals[:, :P].cpu().numpy().T
                a = d.active[:, :P].cpu().numpy().T.astype(bool)
                rows = np.concatenate([_void_rows(hist.vals - shift, hist.active),
                                       _void_rows(v, a)])
                _, index, inverse = np.unique(rows, return_index=True, return_inverse=True)
                first = index[np.asarray(inverse).reshape(-1)][hist.tids.size:]
                mask = first != np.arange(P) + hist.tids.size
                return torch.from_numpy(mask.view(np.uint8)).to(eng.device)

            def suggest(distinct):
                return tpe.suggest_sampled(list(range(K)), domain, trials, SEED,
                                           n_EI_candidates=P, distinct=distinct, verbose=False)

            fns = {"device": run_device, "host": run_host,
                   "suggest_distinct": lambda: suggest(True),
                   "suggest_plain": lambda: suggest(False)}
            times = {n: [] for n in fns}
            last = {}
            # two alternations: the passes, then the suggests (their order swapped
            # every call: the one behind the host route's idle GPU would pay for it)
            for pair in (("device", "host"), ("suggest_distinct", "suggest_plain")):
                for rep in range(args.warmup + args.reps):
                    for n in pair[::-1] if rep % 2 else pair:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        last[n] = fns[n]()
                        torch.cuda.synchronize()
                        if rep >= args.warmup:
                            times[n].append(time.perf_counter() - t0)
            rec = {"space": name, "P": P, "labels": len(labels), "history": int(losses.size),
                   "reps": args.reps}
            for n in fns:
                t = np.sort(times[n])
                rec[n + "_p50_ms"] = 1e3 * float(np.median(t))
                rec[n + "_min_ms"], rec[n + "_max_ms"] = 1e3 * float(t[0]), 1e3 * float(t[-1])
            m_dev = last["device"][:P].cpu().numpy()
            rec["fresh_rows"] = int(P - np.count_nonzero(m_dev))
            rec["same_mask"] = bool(np.array_equal(m_dev, last["host"].cpu().numpy()))
            rec["docs_distinct"], rec["docs_plain"] = (len(last["suggest_distinct"]),
                                                       len(last["suggest_plain"]))
            rec["host_over_device_p50"] = rec["host_p50_ms"] / rec["device_p50_ms"]
            rec["distinct_extra_ms"] = rec["suggest_distinct_p50_ms"] - rec["suggest_plain_p50_ms"]
            results.append(rec)
            print(json.dumps(rec), flush=True)
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
