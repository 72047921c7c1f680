"""The categorical counts' parallel sequential fp64 sum (fold_pass in
hyperopt_amd/csrc/tpe_fold.hpp), restated on the host with Python integers:
it must give the bits of the serial left fold fl(..fl(fl(S + w0) + w1)..)
-- np.bincount's accumulation order (pyll/base.py:1053-1060) -- on LF ramps,
tie-heavy dyadic weights, 24-decade ranges and sums started near 2^53
(tests/fold_cases.py; test_gpu_fold.py runs the device code on the same
lists).  A pass is modelled over its whole list, at both pass sizes: 512
entries (one wave) and 4096 (a block of 8 waves); the scans are written
sequentially (their results do not depend on how a scan is evaluated)."""
import math

import numpy as np

from tests import fold_cases

CAPS = (512, 4096)  # entries per pass: wave scope, block scope


def _split(x):
    """x >= 0 -> (M, biased exponent) with x = M * 2^(max(eb, 1) - 1075)."""
    b = int(np.float64(x).view(np.uint64))
    eb = (b >> 52) & 0x7FF
    M = (b & ((1 << 52) - 1)) | ((1 << 52) if eb else 0)
    return M, eb


def seq_fold(S, w):
    """The kernel's passes over one list (len(w) <= the pass size)."""
    n, r0, passes = len(w), 0, 0
    while r0 < n:
        passes += 1
        A, es = _split(S)
        if S == 0.0 or es == 0:
            S = float(np.float64(S) + np.float64(w[r0]))
            r0 += 1
            continue
        d, tie, huge = [0] * n, [False] * n, [False] * n
        for i in range(r0, n):
            M, ew = _split(w[i])
            sh = es - max(ew, 1)
            if sh < 0:
                huge[i] = True
            elif sh == 0:
                d[i] = M
            elif sh < 64:
                rem, half = M & ((1 << sh) - 1), 1 << (sh - 1)
                d[i] = (M >> sh) + (rem > half)
                tie[i] = rem == half
        P = A & 1  # (the composed parity maps, evaluated in order)
        for i in range(r0, n):
            if tie[i]:
                d[i] += (P + d[i]) & 1
                P = 0
            else:
                P ^= d[i] & 1
        D, cross = 0, None
        for i in range(r0, n):
            if huge[i] or A + D + d[i] >= 1 << 53:
                cross = i
                break
            D += d[i]
        if cross is None:
            S, r0 = math.ldexp(float(A + D), es - 1075), n
        else:
            S = float(np.float64(math.ldexp(float(A + D), es - 1075)) + np.float64(w[cross]))
            r0 = cross + 1
    return S, passes


def _fold_all(S, w, cap):
    for f0 in range(0, len(w), cap):
        S, _ = seq_fold(S, w[f0:f0 + cap])
    return S


def test_lf_ramp_counts_match_the_serial_chain():
    for name, S0, w in fold_cases.lf_ramp_cases():
        want = fold_cases.serial(S0, w)
        for cap in CAPS:
            assert _fold_all(S0, w, cap) == want, (name, cap)


def test_tie_heavy_and_wide_ranges_match_the_serial_chain():
    for name, S0, w in fold_cases.adversarial_cases():
        want = fold_cases.serial(S0, w)
        for cap in CAPS:
            assert _fold_all(S0, w, cap) == want, (name, cap)


def test_passes_stay_few_on_a_long_chain():
    """60 000 ramp weights (a C5 root category): one pass per list plus one
    per binade crossed."""
    rng = np.random.RandomState(5)
    N = 100000
    step = (1.0 - 1.0 / N) / (N - 25 - 1)
    idx = np.sort(rng.choice(N, size=60000, replace=False))
    w = np.where(idx < N - 26, idx * step + 1.0 / N, 1.0).tolist()
    want = fold_cases.serial(0.0, w)
    for cap in CAPS:
        S, total = 0.0, 0
        for f0 in range(0, len(w), cap):
            S, p = seq_fold(S, w[f0:f0 + cap])
            total += p
        assert S == want
        assert total < len(w) / cap + 64
