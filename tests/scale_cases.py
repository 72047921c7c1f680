"""Case table shared by tests/test_scale_cases.py (the oracle alone, no GPU)
and tests/test_gpu_scales.py (the kernels): search spaces far from unit scale.

Every case is an image of one of six canonical cases -- the parameterisations
the rest of the suite uses -- under a map that TPE is equivariant to, so the
oracle's canonical results are a yardstick for the image:

  pow2     bounds, observations, q and candidates times 2^k, k = -20 / +20:
           every mean, bandwidth and candidate is the canonical one times 2^k
           exactly (fp32 and fp64), weights and scores are unchanged
  offset   an affine map x -> a + b x of observations and candidates
  log      the same in log space (t -> a + b t, x = exp t); the quantized log
           kinds have no affine yardstick (q lives in x) and are compared with
           their own image under x -> 2^10 x, q -> 2^10 q
  tiny     images at 2^-40: bandwidths below EPS = 1e-12, where the reference
           itself stops being scale-invariant (max(sigma, EPS),
           max(sqrt2 sigma, EPS)); the device must reproduce the floors.
           fp64 paths only
  outward  a lower bound that fp32 rounds outward ((float)0.7 < 0.7; its log
           twin's (float)low > low), all 25 below observations on `low`

A canonical case is a history of T = 3000 trials (RandomState seeds below),
split by O.ap_split_trials at gamma = 0.25 -- ceil(0.25 sqrt(3000)) = 14 below
observations, 2986 above -- and 2048 injected candidates.  The outward cases
put 25 copies of `low` below instead.

`path` is the route Engine.run takes at precision 32 for drawn candidates:
table (n >= TABLE_MIN_CAND; below it pruned64 with fp32 draws), fp64 (labels
fp32 cannot resolve: the fp64 stream and the exact scorer, at every n), lat
or qfb for quantized labels (with `draw32`: whether the lattice draws in fp32).
tests/test_gpu_scales.py asserts it.
"""
import math
from collections import namedtuple

import numpy as np

from oracle import tpe_oracle as O

T = 3000
GAMMA = 0.25
N_INJ = 2048
KS_N = 200_000      # draws of the distribution checks (CPU: the oracle's sampler; GPU: fp32 stream)
KS_P = 1e-4         # the suite's threshold (tests/test_gpu_sampler.py)

Case = namedtuple("Case", "name kind args below above cand group canon k path draw32 key obs")

_CANON = {
    "U": ("uniform", (-5.0, 5.0), lambda r: r.uniform(-5, 5, T),
          lambda r: r.uniform(-5, 5, N_INJ)),
    "N": ("normal", (0.0, 2.0), lambda r: r.normal(0, 2, T), lambda r: r.normal(0, 3, N_INJ)),
    "QU": ("quniform", (0.0, 100.0, 1.0), lambda r: np.round(r.uniform(0, 100, T)),
           lambda r: np.round(r.uniform(0, 100, N_INJ))),
    "QN": ("qnormal", (0.0, 20.0, 2.0), lambda r: np.round(r.normal(0, 20, T) / 2) * 2,
           lambda r: np.round(r.normal(0, 30, N_INJ) / 2) * 2),
    "LU": ("loguniform", (-5.0, 0.0), lambda r: np.exp(r.uniform(-5, 0, T)),
           lambda r: np.exp(r.uniform(-5, 0, N_INJ))),
    "LN": ("lognormal", (0.0, 1.0), lambda r: np.exp(r.normal(0, 1, T)),
           lambda r: np.exp(r.normal(0, 1.5, N_INJ))),
}
_SEED = {name: 7000 + 10 * i for i, name in enumerate(_CANON)}


def _key(i):
    return (0x5CA1E00000000000 + 0x9E3779B97F4A7C15 * (i + 1)) & 0xFFFFFFFFFFFFFFFF


LOSSES = np.random.RandomState(7001).normal(size=T)   # one history: every case splits alike
IS_BELOW = np.zeros(T, np.uint8)
IS_BELOW[np.argsort(LOSSES, kind="stable")[:min(int(np.ceil(GAMMA * np.sqrt(T))), 25)]] = 1


def _split(obs):
    idx = np.arange(obs.size)
    return O.ap_split_trials(idx, obs, idx, LOSSES, GAMMA)


def _canonical(name):
    kind, args, gen, gen_c = _CANON[name]
    seed = _SEED[name]
    obs = gen(np.random.RandomState(seed))
    cand = gen_c(np.random.RandomState(seed + 2))
    return kind, args, obs, cand


def _build():
    cases = []

    def add(name, kind, args, obs, cand, group, canon, k, path, draw32=None, below=None):
        obs = np.asarray(obs, float)
        b, a = _split(obs)
        assert np.array_equal(b, obs[IS_BELOW == 1]) and np.array_equal(a, obs[IS_BELOW == 0])
        if below is not None:  # (the outward cases: no single history column)
            b, obs = np.asarray(below, float), None
        cases.append(Case(name, kind, tuple(float(a) for a in args), b, a,
                          np.asarray(cand, float), group, canon, k, path, draw32,
                          _key(len(cases)), obs))

    def image(name, canon, kind, args, fx, group, path, k=None, draw32=None):
        _, _, o, c = _canonical(canon)
        add(name, kind, args, fx(o), fx(c), group, canon, k, path, draw32)

    for cn, path in (("U", "table"), ("N", "table"), ("QU", "lat"), ("QN", "lat")):
        kind, args, o, c = _canonical(cn)
        add(cn, kind, args, o, c, "canon", None, 0, path, True if path == "lat" else None)
        for k in (-20, 20):
            s = 2.0 ** k
            add("%s*2^%d" % (cn, k), kind, [v * s for v in args], o * s, c * s, "pow2", cn,
                k, path, True if path == "lat" else None)
    for cn in ("LU", "LN"):
        kind, args, o, c = _canonical(cn)
        add(cn, kind, args, o, c, "canon", None, 0, "table")

    # ---- offsets --------------------------------------------------------------------
    image("uniform(1000,1010)", "U", "uniform", (1000.0, 1010.0), lambda x: 1005.0 + x, "offset",
          "table")
    image("uniform(1e6,1e6+1)", "U", "uniform", (1e6, 1e6 + 1), lambda x: (1e6 + 0.5) + 0.1 * x,
          "offset", "fp64")
    image("normal(1e4,0.5)", "N", "normal", (1e4, 0.5), lambda x: 1e4 + 0.25 * x, "offset",
          "table")
    image("quniform(1e6,1e6+100,1)", "QU", "quniform", (1e6, 1e6 + 100, 1.0),
          lambda x: 1e6 + x, "offset", "lat", draw32=False)
    image("qnormal(1000,50,5)", "QN", "qnormal", (1000.0, 50.0, 5.0), lambda x: 1000.0 + 2.5 * x,
          "offset", "lat", draw32=True)

    # ---- log space ------------------------------------------------------------------
    lo, hi = math.log(1e-6), math.log(1e-1)
    image("loguniform(1e-6,1e-1)", "LU", "loguniform", (lo, hi),
          lambda x: np.exp(lo + (np.log(x) + 5.0) / 5.0 * (hi - lo)), "log", "table")
    image("lognormal(10,0.25)", "LN", "lognormal", (10.0, 0.25),
          lambda x: np.exp(10.0 + 0.25 * np.log(x)), "log", "table")
    r = np.random.RandomState(7100)
    obs = np.round(np.exp(r.uniform(0.0, math.log(1e5), T)))
    add("qloguniform(1,1e5,1)", "qloguniform", (0.0, math.log(1e5), 1.0), obs,
        np.round(np.exp(np.random.RandomState(7102).uniform(0.0, math.log(1e5), N_INJ))), "log",
        None, None, "lat", draw32=False)   # 1e5 slots < LATTICE_CAP: the lattice, fp64 draws
    r = np.random.RandomState(7110)
    obs = np.round(np.exp(r.normal(8.0, 0.5, T)) / 16) * 16
    add("qlognormal(8,0.5,16)", "qlognormal", (8.0, 0.5, 16.0), obs,
        np.round(np.exp(np.random.RandomState(7112).normal(8.0, 0.7, N_INJ)) / 16) * 16, "log",
        None, None, "lat", draw32=None)

    # ---- tiny: the EPS floors (fp64 paths only) -------------------------------------
    s = 2.0 ** -40
    image("uniform(0,10*2^-40)", "U", "uniform", (0.0, 10.0 * s), lambda x: (x + 5.0) * s, "tiny",
          None)
    image("normal(0,2)*2^-40", "N", "normal", (0.0, 2.0 * s), lambda x: x * s, "tiny", None,
          k=-40)

    # ---- bounds fp32 rounds outward -------------------------------------------------
    _, _, o, c = _canonical("U")
    fx = lambda x: 1.0 + 0.06 * x  # noqa: E731
    add("uniform(0.7,1.3)", "uniform", (0.7, 1.3), fx(o), fx(c), "outward", None, None, "table",
        below=np.full(25, 0.7))
    llo, lhi = math.log(0.7), math.log(1.3)
    fl = lambda x: np.exp(llo + (x + 5.0) / 10.0 * (lhi - llo))  # noqa: E731
    add("loguniform(0.7,1.3)", "loguniform", (llo, lhi), fl(o), fl(c), "outward", None, None,
        "table", below=np.full(25, 0.7))
    return cases


CASES = _build()
IDS = [c.name for c in CASES]
BY_NAME = dict(zip(IDS, CASES))
QUANT = [c for c in CASES if c.kind.startswith("q")]
CONT = [c for c in CASES if not c.kind.startswith("q")]
FP32 = [c for c in CONT if c.group != "tiny"]            # cases the fp32 suggest paths run
POW2 = [c for c in CASES if c.group == "pow2"]


def case(name):
    return BY_NAME[name]


def spec(c):
    """(family, prior_mu, prior_sigma, transform, low, high, q) of a case."""
    return O.posterior_spec(c.kind, c.args)


def fits(c, below=None, above=None):
    """The oracle's two posteriors (w, mu, sigma) of a case."""
    fam, pmu, psig, tf, low, high, q = spec(c)
    return tuple(O.adaptive_parzen_normal(tf(np.asarray(o, float)), 1.0, pmu, psig)
                 for o in (c.below if below is None else below,
                           c.above if above is None else above))


def oracle_scores(c, cand=None):
    """The oracle's below - above log-density of a case's candidates."""
    with np.errstate(all="ignore"):
        ref = O.continuous_label_scores(c.kind, c.args, c.below, c.above,
                                        c.cand if cand is None else cand)
    return ref["below_llik"] - ref["above_llik"], ref


def yardstick(c):
    """A case whose scores equal c's in exact arithmetic, candidate by
    candidate: the canonical case where the image is affine in the scoring
    coordinate and keeps the canonical observations; else the case's own image
    under x -> 2^20 x (GMM1) or x -> 2^10 x (LGMM1: a shift of every mean by
    10 log 2; q scaled alike).  None for the tiny cases: the EPS floors break
    the equivariance (see oracle_noise)."""
    if c.group == "tiny":
        return None
    if c.canon is not None:
        return BY_NAME[c.canon]
    fam = spec(c)[0]
    if fam == "GMM1":
        s = 2.0 ** 20
        args = tuple(a * s for a in c.args)
    else:
        s = 2.0 ** 10
        shifted = 1 if c.kind in ("lognormal", "qlognormal") else 2  # mu / both log bounds
        args = tuple(a + math.log(s) for a in c.args[:shifted]) + c.args[shifted:2] + \
            tuple(a * s for a in c.args[2:])
    return c._replace(name=c.name + "~", args=args, below=c.below * s, above=c.above * s,
                      cand=c.cand * s, canon=None, obs=None)


_noise = {}


def oracle_noise(c):
    """Largest disagreement of the oracle with itself between a case and its
    yardstick, over the case's candidates: the rounding the oracle carries at
    the case's magnitude.  A tiny case takes the figure of its canonical
    case's 2^-20 image: its values are centred on zero like that image's, so
    the same operations round alike, floors or not."""
    if c.name not in _noise:
        if c.group == "tiny":
            _noise[c.name] = oracle_noise(BY_NAME["%s*2^-20" % c.canon])
        elif c.group == "canon":
            _noise[c.name] = max(oracle_noise(BY_NAME["%s*2^%d" % (c.name, k)])
                                 for k in (-20, 20)) if c.name in ("U", "N", "QU", "QN") \
                else oracle_noise(c._replace(group="self", canon=None))
        else:
            s, _ = oracle_scores(c)
            y, _ = oracle_scores(yardstick(c))
            ok = np.isfinite(s) & np.isfinite(y)
            assert np.array_equal(np.isfinite(s), np.isfinite(y)), c.name
            _noise[c.name] = float(np.max(np.abs(s[ok] - y[ok]))) if ok.any() else 0.0
    return _noise[c.name]


def in_support(c, x):
    """Candidates inside [low, high) ([exp low, exp high) for log kinds).  A
    quantized draw is accepted there and then rounded to its lattice point
    (tpe.py:79-106), so it lies within q / 2 of that range, `high` included."""
    fam, _, _, _, low, high, q = spec(c)
    if low is None:
        return np.ones(np.shape(x), bool)
    if fam == "LGMM1":
        low, high = math.exp(low), math.exp(high)
    if q is not None:
        return (low - q / 2 <= x) & (x <= high + q / 2)
    return (low <= x) & (x < high)


def on_lattice(c, x):
    q = spec(c)[6]
    return np.rint(x / q) * q == x
