"""Case table and comparison rules shared by tests/test_oracle_streams.py (the
replay alone, no GPU) and tests/test_gpu_streams.py (the kernels against the
replay, oracle/streams.py).

A case is an explicit 1-D mixture with bounds and a Philox key.  The
tolerances and the ambiguity rules live here so that both files apply the
same ones: a candidate whose replayed attempt lies within the comparison
tolerance of a bound may be accepted by one side and rejected by the other; it
is skipped, and the number of such candidates per case is capped (asserted
from the replay alone on the CPU, so a cap cannot hide a kernel error).
"""
from collections import namedtuple

import numpy as np

from oracle import streams as S
from oracle import tpe_oracle as O

N_CAND = 2 * 4096 + 1021   # several blocks, a partial wave, a thread with < 16 valid slots
BASES = (0, 5, 2 ** 32 - 2050, 2 ** 40 + 1)  # aligned, unaligned, across / far above 2^32
WAVE_CAND = 1024            # candidates of one wave of the fp32 sampler (64 lanes x 16)
RETRY_LIST = 256            # rejections a wave lists before a lane keeps its own

RTOL64 = 1e-13              # fp64 draw formulas (test_gpu_anneal's rtol)
RTOL32 = 1e-4               # the project's fp32 parity tolerance
CAP64 = 2                   # ambiguous candidates per case, fp64 stream
CAP32 = 0.01                # ... fp32 stream: a fraction of the case's candidates
CAP_Q = 0.01                # quantized: lattice indices next to a half-integer

Case = namedtuple("Case", "name family w mu sigma low high key n tag")


def _key(i):
    return (0x5DEECE66D1234567 + 0x9E3779B97F4A7C15 * (i + 1)) & 0xFFFFFFFFFFFFFFFF


def _fits():
    """adaptive_parzen_normal fits of n_obs observations: 1, 2, 26, 64, 65 and
    301 components -- both sides of the sampler's staging limit (64)."""
    kinds = [("uniform", (-5.0, 5.0), lambda r, n: r.uniform(-5, 5, n)),
             ("normal", (0.0, 2.0), lambda r, n: r.normal(0, 2, n)),
             ("loguniform", (-5.0, 0.0), lambda r, n: np.exp(r.uniform(-5, 0, n)))]
    out = []
    for kind, args, gen in kinds:
        fam, pmu, psig, tf, low, high, _ = O.posterior_spec(kind, args)
        for n_obs in (0, 1, 25, 63, 64, 300):
            rng = np.random.RandomState(1000 + n_obs)
            w, mu, sig = O.adaptive_parzen_normal(tf(gen(rng, n_obs)), 1.0, pmu, psig)
            out.append(Case("%s-%d" % (kind, n_obs), fam, w, mu, sig, low, high, _key(len(out)),
                            N_CAND, "fit"))
    return out


def _special(i0):
    # ten weights of 1e-4 among large ones, some adjacent: guide buckets that
    # hold a second (and third) threshold
    w = np.ones(40)
    w[[3, 4, 5, 11, 12, 20, 21, 22, 23, 30]] = 1e-4
    multi = Case("multi", "GMM1", w, np.linspace(-4.0, 4.0, 40), np.full(40, 0.3), -5.0, 5.0,
                 _key(i0), N_CAND, "multi")
    # half of the mass below `low`: > 25 % of a wave rejected, its list overflows
    half = Case("half", "GMM1", np.ones(5), np.array([-1.0, -0.4, 0.0, 0.4, 1.0]),
                np.full(5, 0.5), 0.0, 6.0, _key(i0 + 1), N_CAND, "half")
    # ~97 % rejected: several retry calls per candidate, some reach the clamp
    r97 = Case("r97", "GMM1", np.ones(3), np.array([-0.2, 0.0, 0.2]), np.ones(3), 1.9, 2.5,
               _key(i0 + 2), N_CAND, "r97")
    # every component ~40 sigma outside, on both sides: every attempt rejected
    clamp = Case("clamp", "GMM1", np.ones(3), np.array([-41.0, -40.0, 45.0]), np.ones(3), 0.0,
                 1.0, _key(i0 + 3), 257, "clamp")
    return [multi, half, r97, clamp]


CASES = _fits()
CASES += _special(len(CASES))
CASE_IDS = [c.name for c in CASES]

# quantized cases: (case name, q)
QUANT = [("uniform-25", 1.0), ("normal-25", 0.5), ("loguniform-25", 0.05), ("half", 0.25)]


def case(name):
    return CASES[CASE_IDS.index(name)]


def host_cdf(c):
    """The mixture as _Mixture holds it (sorted by mean), with a host-side
    cumulative weight -- for the CPU file; the GPU file replays from the
    device's own cdf."""
    order = np.argsort(c.mu, kind="stable")
    w = np.asarray(c.w, np.float64)[order]
    return np.cumsum(w) / w.sum(), np.asarray(c.mu)[order], np.asarray(c.sigma)[order]


def indices(c, base):
    return base + np.arange(c.n, dtype=np.int64)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def _bound_ulp32(c):
    b = [abs(v) for v in (c.low, c.high) if v is not None]
    return float(ulp32(max(b))) if b else 0.0


# ---------------------------------------------------------------------------
# ambiguity (from the replay alone)
# ---------------------------------------------------------------------------
def ambiguous64(c, rep):
    """fp64: an attempt within RTOL64 (|mu_k| + sigma_k max(1, |z|)) of a bound."""
    return rep["near"] <= RTOL64


def ambiguous32(c, rep):
    """fp32: an attempt within RTOL32 sigma_k max(1, |z|) + 2 ulp32 of a bound
    (the ulp term taken at the larger bound, over the smallest sigma)."""
    return rep["near"] <= RTOL32 + 2.0 * _bound_ulp32(c) / float(np.min(rep["sigma32"]))


def tol64(rep, mu, sigma):
    k, z = rep["comp"], rep["z"]
    return RTOL64 * (np.abs(mu[k]) + np.abs(sigma[k]) * np.maximum(1.0, np.abs(z)))


def tol32(rep, y_dev):
    k, z = rep["comp"], rep["z"]
    return RTOL32 * rep["sigma32"][k] * np.maximum(1.0, np.abs(z)) + 2.0 * ulp32(y_dev)


# ---------------------------------------------------------------------------
# quantized slots
# ---------------------------------------------------------------------------
def quant_index(c, rep, q, tol_y, fast_exp):
    """(lattice index rint(v / q) of the replayed draw, ambiguous): v = y, or
    exp(y) for LGMM1.  Ambiguous: v / q within the stream's tolerance of a
    half-integer -- tol_y in y, carried through exp for LGMM1, plus (fp32
    stream) the error of the fast exp2-based exponential: its argument
    y log2(e) is rounded to fp32 and the instruction is good to an ulp, a
    relative error below 4 * 2^-24 * max(1, |y|)."""
    y = rep["y"]
    if c.family == "LGMM1":
        v = np.exp(y)
        tol_v = v * np.expm1(tol_y)
        if fast_exp:
            tol_v = tol_v + v * 4.0 * 2.0 ** -24 * np.maximum(1.0, np.abs(y))
    else:
        v, tol_v = y, tol_y
    s = v / q
    k = np.rint(s)
    half = np.abs(np.abs(s - np.floor(s)) - 0.5) * q  # distance of v to the nearest half-step
    return k.astype(np.int64), half <= tol_v + 4.0 * np.spacing(np.abs(v))


# ---------------------------------------------------------------------------
# paths a case is named for (from the replay's call counts)
# ---------------------------------------------------------------------------
def max_wave_rejections(rep, per_wave=WAVE_CAND):
    """Largest number of first-attempt rejections in one wave's candidates
    (consecutive runs of per_wave local indices)."""
    r = rep["rejected0"]
    return max(int(r[i:i + per_wave].sum()) for i in range(0, r.size, per_wave))


def multi_buckets(cdf):
    """Guide buckets (top 8 bits of a word) that hold two or more thresholds."""
    thr = S.thresholds(cdf)[:-1]
    return int(np.sum(np.bincount((thr >> np.uint64(24)).astype(np.int64), minlength=256) >= 2))


# ---------------------------------------------------------------------------
# prior draws
# ---------------------------------------------------------------------------
PRIOR_SEED = 123
PRIOR_N = 1000
PRIOR_BASES = (0, 2 ** 32 - 5)
CAP_PRIOR = 2               # quantized log / normal draws next to a half-integer, per label


def prior_records():
    """(labels, tpe_prior records with keys, probability pool) of the
    eleven-label space of test_prior_draws_match_reference_distributions plus
    uniform(0, 1), whose draw is u01_f64 itself."""
    from hyperopt_amd import hp
    from hyperopt_amd.base import Domain
    from hyperopt_amd.rand import _prior_table
    from hyperopt_amd.tpe import label_keys
    space = {
        "u": hp.uniform("u", -3, 4), "lu": hp.loguniform("lu", -2, 1),
        "n": hp.normal("n", 1, 2), "ln": hp.lognormal("ln", 0.5, 0.7),
        "qu": hp.quniform("qu", 0, 10, 3), "qlu": hp.qloguniform("qlu", 0, 3, 2),
        "qn": hp.qnormal("qn", 0, 10, 2), "qln": hp.qlognormal("qln", 0, 1, 0.5),
        "ri": hp.randint("ri", 10), "ri2": hp.randint("ri2", 12, 25),
        "pc": hp.pchoice("pc", [(0.1, "a"), (0.3, "b"), (0.6, "c")]),
        "u01": hp.uniform("u01", 0, 1),
    }
    labels, rec, pool = _prior_table(Domain(lambda p: 0.0, space))
    rec = rec.copy()
    rec["key"] = label_keys(PRIOR_SEED, labels)
    return labels, rec, pool


def prior_is_smooth(R):
    """Kinds that go through log / exp / Box-Muller (compared within a
    tolerance); the others are the same IEEE operations in numpy (exact)."""
    return int(R["kind"]) in (S.PRIOR_LOGUNIFORM, S.PRIOR_NORMAL, S.PRIOR_LOGNORMAL)


def prior_tol(R, d):
    """Tolerance of a smooth kind's unquantized value: RTOL64 of the
    magnitude of its terms before exp (|a| + |b| max(1, |z|); the uniform
    part is exact), carried through exp as a relative error."""
    a, b = float(R["a"]), float(R["b"])
    scale = 1.0 if d["z"] is None else abs(a) + abs(b) * np.maximum(1.0, np.abs(d["z"]))
    return RTOL64 * scale * (np.abs(d["raw"]) if int(R["kind"]) != S.PRIOR_NORMAL else 1.0)


def prior_half(R, d):
    """Quantized smooth kinds: draws whose raw / q lies within prior_tol of a
    half-integer."""
    q, raw = float(R["q"]), d["raw"]
    s = raw / q
    return np.abs(np.abs(s - np.floor(s)) - 0.5) * q <= prior_tol(R, d) + 4 * np.spacing(
        np.abs(raw))


# ---------------------------------------------------------------------------
# annealing
# ---------------------------------------------------------------------------
ANNEAL_ROWS, ANNEAL_TRIALS = 257, 96
ANNEAL_IDS = 2 ** 32 - 48 + np.arange(ANNEAL_TRIALS, dtype=np.int64)  # across 2^32
ANNEAL_AVG = (2.0, 1000.0)
ANNEAL_KINDS = (S.PRIOR_UNIFORM, S.PRIOR_NORMAL, S.PRIOR_UNIFORM)
ANNEAL_QUOTIENT_TOL = 1e-12  # an id whose quotient is this close to an integer is skipped: cap 0


def anneal_history():
    """(losses, active, vals, label keys): 257 rows with ties, +inf and NaN
    losses; a full column, every third row, and three rows only.  Trial t
    draws label t % 3."""
    from hyperopt_amd.tpe import label_keys_array
    rng = np.random.RandomState(ANNEAL_ROWS)
    losses = rng.normal(size=ANNEAL_ROWS).round(1)
    losses[rng.rand(ANNEAL_ROWS) < 0.05] = np.inf
    losses[rng.rand(ANNEAL_ROWS) < 0.05] = np.nan
    active = np.zeros((ANNEAL_ROWS, 3), bool)
    active[:, 0] = True
    active[::3, 1] = True
    active[rng.choice(ANNEAL_ROWS, 3, replace=False), 2] = True
    vals = np.where(active, rng.uniform(0, 1, active.shape), np.nan)
    return losses, active, vals, label_keys_array(7, ["a", "b", "c"])
