"""The categorical posteriors at the shapes DESIGN.md 3.2.1 quotes, launched
3 + 20 times each, for a kernel trace of the count / fold kernels:

  history 10 000 rows x 8 categories    k_cat_counts_hist
  history 100 000 x 3                   k_cath_count / k_cath_emit / k_cath_fold
  history 100 000 x 40                  k_cat_counts_hist (more than 32 categories)
  uploaded lists 60 000 x 3             k_cat_counts

One label, the above set (the below set's 25 rows ride along).  Per-kernel
times come from a kernel trace of this program run on its own (no counters;
the program after `--`):

  rocprofv3 --kernel-trace --stats -d out -- python tools/probes/cat_probe.py

Without a profiler it prints the host time per posterior call, which is
launch overhead and copies as much as kernels."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

WARMUP, CALLS = 3, 20
SHAPES = [("hist", 10_000, 8), ("hist", 100_000, 3), ("hist", 100_000, 40), ("lists", 60_000, 3)]


def main():
    import torch
    from hyperopt_amd.engine import DeviceHistory, Engine, LabelWork
    torch.cuda.set_device(0)
    eng = Engine()
    for mode, T, K in SHAPES:
        rng = np.random.RandomState(T + K)
        p = rng.dirichlet(np.full(K, 0.5))
        col = rng.choice(K, size=T, p=p)
        isb = np.zeros(T, np.uint8)
        isb[np.argsort(rng.normal(size=T), kind="stable")[:25]] = 1
        spec = ("c", "categorical", (tuple(p.tolist()),))
        if mode == "hist":
            hist = DeviceHistory(eng, 1)
            hist.append(col.astype(float)[:, None], np.ones((T, 1), bool))
            work = LabelWork(*spec, col[isb == 1].astype(float), None, col=0, n_above=T - 25)
            kw = dict(history=hist, is_below=isb)
        else:
            work = LabelWork(*spec, col[isb == 1], col[isb == 0])
            kw = {}
        ts = []
        for _ in range(WARMUP + CALLS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r, = eng.run([work], posteriors=True, **kw)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ms = np.array(ts[WARMUP:]) * 1e3
        print("%-5s %7d x %2d  host ms per call: median %.3f min %.3f  p_above[0] %r"
              % (mode, T, K, np.median(ms), ms.min(), float(r.extra["p_above"][0])), flush=True)


if __name__ == "__main__":
    main()
