#!/usr/bin/env python
"""Times ``joint="tree"`` (one joint Parzen mixture per group of labels that
share an activation condition) on a conditional space of C3's
size: a 4-way root choice ``v`` and the 50 C3 labels under its branches (label
i under branch i % 4: 13, 13, 12 and 12 labels), with a 10k-trial history whose
trials take the four branches uniformly.

  (a) whole calls, host clock, the copy of S to the host included (it is what
      synchronises): tpe.score_configs(joint="tree") against joint=True on the
      same pool -- joint=True is the path as it was: J of the selector alone
      plus the factorised terms of the live labels;
  (b) the list scorer by itself, between device events: tpe_joint_score_rows
      on the identity list against tpe_joint_score on the same rows and set
      (what the gather and the device-side count cost), and on a 1-in-4 list
      against the dense call on all the rows (what the list saves).  The set is
      the above set of the first branch's group; the rows are dense draws of
      its labels.

The compared paths alternate in one process; --warmup calls, then the p50
(min-max) of --reps.  One JSON line per pool size.

    python tools/probes/joint_tree_probe.py [--log2 12 16] [--reps 7]
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

BRANCHES = 4


def tree_space(space):
    """(hp space, {label: branch}) of the C3 labels under a 4-way choice."""
    from hyperopt_amd import hp
    branch = {lab: i % BRANCHES for i, (lab, _, _) in enumerate(space)}
    node = {lab: (hp.randint(lab, a[0]) if kind == "randint" else getattr(hp, kind)(lab, *a))
            for lab, kind, a in space}
    opts = [{lab: node[lab] for lab in node if branch[lab] == b} for b in range(BRANCHES)]
    return {"v": hp.choice("v", opts)}, branch


def tree_trials(domain, space, branch, vals, losses):
    """The C3 history with trial i on branch v_i (seed 2): a trial holds the
    labels of its branch only."""
    from hyperopt_amd import Trials
    from hyperopt_amd.base import JOB_STATE_DONE
    T = losses.size
    v = np.random.RandomState(2).randint(0, BRANCHES, T)
    ints = {lab for lab, kind, _ in space if kind == "randint"}
    cols = {lab: (vals[lab].astype(np.int64).tolist() if lab in ints else vals[lab].tolist())
            for lab, _, _ in space}
    miscs = []
    for i in range(T):
        on = {lab: branch[lab] == v[i] for lab in cols}
        idxs = {lab: [i] if on[lab] else [] for lab in cols}
        vs = {lab: [cols[lab][i]] if on[lab] else [] for lab in cols}
        idxs["v"], vs["v"] = [i], [int(v[i])]
        miscs.append({"tid": i, "cmd": domain.cmd, "workdir": None, "idxs": idxs, "vals": vs})
    trials = Trials()
    docs = trials.new_trial_docs(list(range(T)), [None] * T,
                                 [{"status": "ok", "loss": float(x)} for x in losses], miscs)
    for d in docs:
        d["state"] = JOB_STATE_DONE
    trials.insert_trial_docs(docs)
    trials.refresh()
    return trials


def dense_draws(domain, space, P, seed=7):
    """(P, L) prior draws of every label (``v`` included), nothing masked
    (pool_probe.c3_pool's draw rules)."""
    rng = np.random.RandomState(seed)
    kinds = {lab: (kind, a) for lab, kind, a in space}
    kinds["v"] = ("randint", (BRANCHES,))
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
    return np.stack(cols, 1)


def stats(times, name, rec, unit=1e3):
    t = np.sort(np.asarray(times))
    rec[name + "_p50_ms"] = unit * float(np.median(t))
    rec[name + "_min_ms"], rec[name + "_max_ms"] = unit * float(t[0]), unit * float(t[-1])


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
        sys.exit("joint_tree_probe needs a GPU")
    import bench
    from hyperopt_amd import _lib as L
    from hyperopt_amd import joint as J
    from hyperopt_amd import pool as pool_mod
    from hyperopt_amd import tpe
    from hyperopt_amd.base import Domain

    space = bench.c3_space()
    vals, losses = bench.c3_history(space)
    hps, branch = tree_space(space)
    domain = Domain(lambda p: 0.0, hps)
    labels = list(domain.params)
    trials = tree_trials(domain, space, branch, vals, losses)
    groups = J.joint_groups(domain)
    eng = tpe.engine()
    lib = L.load()
    kw = dict(prior_weight=1.0, gamma=0.25, linear_forgetting=25)
    results = []
    for lg in args.log2:
        P = 1 << lg
        draws = dense_draws(domain, space, P)
        v = draws[:, labels.index("v")].astype(np.int64)
        active = np.stack([np.ones(P, bool) if lab == "v" else branch[lab] == v
                           for lab in labels], 1)
        pool = tpe.Pool.from_arrays(domain, draws, active)
        rec = {"P": P, "labels": len(labels), "groups": [len(g.labels) for g in groups],
               "history": int(losses.size), "reps": args.reps, "warmup": args.warmup,
               "chunk": int(lib.tpe_joint_chunk()), "rows_per_call": J.ROWS_PER_CALL}

        # (a) the whole public call
        fns = {"tree": lambda: tpe.score_configs(domain, trials, pool, joint="tree", **kw),
               "joint_true": lambda: tpe.score_configs(domain, trials, pool, joint=True, **kw)}
        times = {n: [] for n in fns}
        for rep in range(args.warmup + args.reps):
            for n in fns:  # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fns[n]()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    times[n].append(time.perf_counter() - t0)
        for n in fns:
            stats(times[n], n, rec)
        rec["tree_over_joint_true_p50"] = rec["tree_p50_ms"] / rec["joint_true_p50_ms"]

        # (b) the list scorer by itself, on dense draws of the first branch's group
        hist = tpe.collect_history(trials, labels)
        grp = groups[1]
        fit = J.fit(eng, domain, hist, pool_mod._seen_rows(eng, hist), kw["gamma"], len(labels),
                    1.0, 25, J.BANDWIDTH, J.CAT_SMOOTHING, tree=True)[1]
        assert fit.group == grp.labels
        dj, sets, sp = fit.dj, fit.sets, fit.sp
        dset, n, _ = sets[1]
        rec["b_labels"], rec["b_components"] = len(grp.labels), n + 1
        dev = eng.device
        d_vals = torch.from_numpy(np.ascontiguousarray(draws.T)).to(dev)
        out = torch.empty(P, dtype=torch.float64, device=dev)
        scratch = torch.empty(lib.tpe_joint_scratch_bytes(P, n), dtype=torch.uint8, device=dev)
        tab = None if dj.tables is None else dj.tables.data_ptr()
        head = (dj.host.ctypes.data, dj.dev.data_ptr(), len(dj.models), tab, dj.n_tables,
                dset.data_ptr(), n, d_vals.data_ptr(), P, len(labels))
        lists = {"identity": np.arange(P, dtype=np.int64),
                 "quarter": np.arange(0, P, 4, dtype=np.int64)}
        d_lists = {k: (torch.from_numpy(a).to(dev),
                       torch.from_numpy(np.asarray([a.size], np.int64)).to(dev))
                   for k, a in lists.items()}

        def dense():
            L.check(lib.tpe_joint_score(*head, 0, P, None, out.data_ptr(), scratch.data_ptr(),
                                        sp), "tpe_joint_score")

        def by_list(name):
            rows, count = d_lists[name]
            L.check(lib.tpe_joint_score_rows(*head, rows.data_ptr(), count.data_ptr(), 0, P, None,
                                             out.data_ptr(), 0, scratch.data_ptr(), sp),
                    "tpe_joint_score_rows")

        kernels = {"dense": dense, "list_identity": lambda: by_list("identity"),
                   "list_quarter": lambda: by_list("quarter")}
        ktimes = {k: [] for k in kernels}
        for rep in range(args.warmup + args.reps):
            for k, fn in kernels.items():  # alternating
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rep >= args.warmup:
                    ktimes[k].append(e0.elapsed_time(e1))
        for k in kernels:
            stats(ktimes[k], "b_" + k, rec, unit=1.0)
        rec["b_identity_over_dense_p50"] = rec["b_list_identity_p50_ms"] / rec["b_dense_p50_ms"]
        rec["b_quarter_over_dense_p50"] = rec["b_list_quarter_p50_ms"] / rec["b_dense_p50_ms"]
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del pool, d_vals, out, scratch
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
