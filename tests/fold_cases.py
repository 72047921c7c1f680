"""Lists for the categorical counts' exact fold (hyperopt_amd/csrc/tpe_fold.hpp)
and their reference, the serial chain s = s + w in numpy float64 --
np.bincount's accumulation order (pyll/base.py:1053-1060).  Shared by the
host restatement (test_seq_fold.py) and the device run (test_gpu_fold.py);
each case is (name, start value, weights), built once per process."""
import functools

import numpy as np

STARTS = [0.0, 1.0, 2.0 ** 53, 2.0 ** 53 + 2, 2.0 ** 52 + 1, 3 * 2.0 ** 51 + 1, 1e16, 1e-300]
KINDS = ("dyadic-mix", "dyadic-ties", "24-decades")


def serial(S, w):
    """The reference: fl(..fl(fl(S + w0) + w1)..), independent of any fold."""
    s = np.float64(S)
    for x in w:
        s = s + np.float64(x)
    return float(s)


def weights(rng, kind, n):
    """The three adversarial weight kinds, one rng draw per entry."""
    if kind == 0:
        return [float(rng.choice([1.0, 3.0, 0.5, 2.0, 1.5, 5.0, 2.0 ** -60, 7.0, 0.0]))
                for _ in range(n)]
    if kind == 1:
        return [float(2.0 ** rng.randint(-6, 3)) * int(rng.randint(1, 4)) for _ in range(n)]
    return [float(10.0 ** rng.uniform(-12, 12)) for _ in range(n)]


def two_category_column(n, m):
    """n observations of two categories, exactly m of category 0, the others
    (category 1) spread evenly through the column: a chain of a chosen length
    for the engine paths (the serial prefix ends after 4096 matches)."""
    col = np.zeros(n, np.int64)
    col[np.round(np.linspace(0, n - 1, n - m)).astype(np.int64)] = 1
    assert int((col == 0).sum()) == m
    return col


@functools.lru_cache(maxsize=None)
def lf_ramp_cases():
    """Matches of a category on linear-forgetting ramps (tpe.py:380-392)."""
    rng = np.random.RandomState(3)
    out = []
    for N in (30, 1000, 20000):
        lf = 25
        num = N - lf
        step = (1.0 - 1.0 / N) / (num - 1)
        for p in (0.05, 0.5, 0.9):
            idx = np.flatnonzero(rng.uniform(size=N) < p)
            w = np.where(idx < num - 1, idx * step + 1.0 / N, 1.0).tolist()
            out.append(("ramp N=%d p=%g" % (N, p), 0.0, w))
    return out


@functools.lru_cache(maxsize=None)
def adversarial_cases():
    """Tie-heavy dyadic weights and 24-decade ranges, sums started at 0, 1,
    around 2^53 / 2^52, 1e16 and 1e-300."""
    rng = np.random.RandomState(4)
    out = []
    for trial in range(400):
        n = int(rng.randint(1, 1500))
        kind = trial % 3
        w = weights(rng, kind, n)
        S0 = float(STARTS[trial % len(STARTS)])
        out.append(("trial %d %s n=%d S0=%r" % (trial, KINDS[kind], n, S0), S0, w))
    return out


@functools.lru_cache(maxsize=None)
def edge_cases(lengths):
    """Every weight kind at each list length (a pass's or a staged chunk's
    edge), the start values taken in turn, and one subnormal start."""
    rng = np.random.RandomState(6)
    out = []
    for i, n in enumerate(lengths):
        for kind in range(3):
            if kind == 0:
                w = rng.choice([1.0, 3.0, 0.5, 2.0, 1.5, 5.0, 2.0 ** -60, 7.0, 0.0], size=n)
            elif kind == 1:
                w = 2.0 ** rng.randint(-6, 3, size=n) * rng.randint(1, 4, size=n)
            else:
                w = 10.0 ** rng.uniform(-12, 12, size=n)
            S0 = float(STARTS[(3 * i + kind) % len(STARTS)])
            out.append(("edge n=%d %s S0=%r" % (n, KINDS[kind], S0), S0, w.tolist()))
    w = rng.choice([2.0 ** -1074, 2.0 ** -1060, 0.0, 2.0 ** -1022, 1.0, 0.5], size=700)
    out.append(("subnormal start", 5e-324, w.tolist()))
    return out
