#!/usr/bin/env python
"""Times the chain term of ``joint="chain"`` on the suite's
``nested`` space: P pool rows and a T-trial history, both sampled from the
prior with seeded uniform losses.

Per group with a context and per set, log L - log L_ctx of the group's live
rows is formed two ways, between device events, alternating in one process:

  fused     tpe_joint_chain_rows: one walk over the labels ctx + g that joins
            the context's (m, s) at the label boundary;
  two_call  tpe_joint_score_rows on the same set, and tpe_joint_score_rows with
            n_labels = n_ctx on a set that tpe_joint_prep builds from the
            context's labels with the full set's sigmas (what the entry points
            gave before tpe_joint_chain_rows; the subtraction of the two
            vectors is not timed).

Before timing, the two forms' values are compared bit for bit.  --warmup
calls, then the p50 (min-max) of --reps.  One JSON line.

    python tools/probes/joint_chain_probe.py [--log2 14] [--trials 10000] [--reps 15]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def context_set(lib, L, torch, fit, ctx_dj, seen, n_cols, which):
    """The set of ``fit.sets[which]`` over the first n_ctx labels alone: the
    full set's log w and sigmas, the components by tpe_joint_prep."""
    full, n, drows = fit.sets[which]
    D, k, C = len(fit.dj.models), fit.n_ctx, n + 1
    dset = torch.empty(lib.tpe_joint_set_doubles(k, n), dtype=torch.float64, device=full.device)
    dset[:C].copy_(full[:C])
    dset[C:C + k].copy_(full[C:C + k])
    dset[C + k:C + 2 * k].copy_(full[C + D:C + D + k])
    _alive, sv, sa, sld, _rows, _T = seen
    L.check(lib.tpe_joint_prep(ctx_dj.host.ctypes.data, ctx_dj.dev.data_ptr(), k, sv, sa, sld,
                               n_cols, None if drows is None else drows.data_ptr(), n,
                               dset.data_ptr(), fit.sp), "tpe_joint_prep")
    return dset


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2", type=int, default=14, help="pool size (log2 P)")
    ap.add_argument("--trials", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", help="also write the JSON result here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("joint_chain_probe needs a GPU")
    from hyperopt_amd import _lib as L
    from hyperopt_amd import hp, rand, tpe
    from hyperopt_amd import joint as J
    from hyperopt_amd import pool as pool_mod
    from hyperopt_amd.base import Domain
    from tests import joint_util as U
    from tests.golden import spaces

    domain = Domain(lambda p: 0.0, spaces.SPACES["nested"](hp))
    labels = list(domain.params)
    rng = np.random.RandomState(1)
    T, P = args.trials, 1 << args.log2
    trials = U.make_trials(domain, [rand.sample_config(domain, rng) for _ in range(T)],
                           rng.uniform(size=T))
    pool = tpe.Pool(domain, [rand.sample_config(domain, rng) for _ in range(P)])
    eng, lib = tpe.engine(), L.load()
    dev = eng.device
    hist = tpe.collect_history(trials, labels)
    seen = pool_mod._seen_rows(eng, hist)
    n_cols = len(labels)
    fits = [f for f in J.fit(eng, domain, hist, seen, 0.25, n_cols, 1.0, 25, J.BANDWIDTH,
                             J.CAT_SMOOTHING, tree="chain") if f.n_ctx]
    d = pool.device(eng)
    ld = int(d.vals.shape[1])
    rec = {"P": P, "history": T, "reps": args.reps, "warmup": args.warmup,
           "chunk": int(lib.tpe_joint_chunk()), "groups": []}

    work = []  # per (group, set): the arguments of the three calls
    cscratch = torch.empty(lib.tpe_rows_compact_scratch_bytes(P), dtype=torch.uint8, device=dev)
    n_max = max(n for f in fits for _, n, _ in f.sets)
    scratch = torch.empty(lib.tpe_joint_chain_scratch_bytes(P, n_max), dtype=torch.uint8,
                          device=dev)
    for f in fits:
        k, D = f.n_ctx, len(f.dj.models)
        ctx_dj = J._device_labels(eng, f.dj.models[:k], f.cat_smoothing)
        lst = torch.empty(P, dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        L.check(lib.tpe_rows_compact(d.active.data_ptr() + f.dj.models[k].col * ld, P,
                                     lst.data_ptr(), count.data_ptr(), cscratch.data_ptr(), f.sp),
                "tpe_rows_compact")
        rec["groups"].append({"labels": f.group, "n_ctx": k, "D": D, "live_rows": int(count.item()),
                              "components": [n + 1 for _, n, _ in f.sets]})
        for which in (0, 1):
            full, n, _ = f.sets[which]
            cset = context_set(lib, L, torch, f, ctx_dj, seen, n_cols, which)

            def head(dj, n_labels, dset, n=n):
                tab = None if dj.tables is None else dj.tables.data_ptr()
                return (dj.host.ctypes.data, dj.dev.data_ptr(), n_labels, tab, dj.n_tables,
                        dset.data_ptr(), n, d.vals.data_ptr(), ld, n_cols)
            tail = (lst.data_ptr(), count.data_ptr(), 0, P, None)
            outs = [torch.zeros(P, dtype=torch.float64, device=dev) for _ in range(3)]
            hf = head(f.dj, D, full)
            work.append(dict(
                keep=(ctx_dj, cset, lst, count), outs=outs, sp=f.sp,
                fused=hf[:3] + (k,) + hf[3:] + tail,
                full=hf + tail, ctx=head(ctx_dj, k, cset) + tail))

    def fused():
        for w in work:
            L.check(lib.tpe_joint_chain_rows(*w["fused"], w["outs"][0].data_ptr(), 0,
                                             scratch.data_ptr(), w["sp"]), "tpe_joint_chain_rows")

    def two_call():
        for w in work:
            for name, o in (("full", 1), ("ctx", 2)):
                L.check(lib.tpe_joint_score_rows(*w[name], w["outs"][o].data_ptr(), 0,
                                                 scratch.data_ptr(), w["sp"]),
                        "tpe_joint_score_rows")

    fused()
    two_call()
    torch.cuda.synchronize()
    same = True
    for w in work:
        a, b, c = (o.cpu().numpy() for o in w["outs"])
        with np.errstate(invalid="ignore"):
            want = b - c
        nan = np.isnan(want)
        same &= bool((np.isnan(a) == nan).all() and
                     (a[~nan].view(np.uint64) == want[~nan].view(np.uint64)).all())
    rec["same_bits"] = same

    forms = {"fused": fused, "two_call": two_call}
    times = {k: [] for k in forms}
    for rep in range(args.warmup + args.reps):
        for k, fn in forms.items():  # alternating
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                times[k].append(e0.elapsed_time(e1))
    for k in forms:
        t = np.sort(np.asarray(times[k]))
        rec[k + "_p50_ms"], rec[k + "_min_ms"], rec[k + "_max_ms"] = \
            float(np.median(t)), float(t[0]), float(t[-1])
    rec["fused_over_two_call_p50"] = rec["fused_p50_ms"] / rec["two_call_p50_ms"]
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
