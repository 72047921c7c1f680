"""Case table shared by tests/test_lattice_cases.py (the oracle and the numpy
replay of the streams alone, no GPU) and tests/test_gpu_lattice_stages.py (the
kernels of csrc/tpe_quantized.hip stage by stage).

A case is a quantized label with a history and a Philox key, small enough to
run in a few tiles: N_FULL = 3 tiles and 77 candidates, the prefix one tile.
It names the route the label takes at precision 32:

  draw     "pow2"   k_lattice_sample<POW2>: fp32 draws, q a power of two, at most
                    K_LAT_LDS slots
           "gen32"  the general instantiation on fp32 draws (the `mark` lambda
                    in fp64 on the converted draw)
           "gen64"  the general instantiation on fp64 draws (a slot index past
                    DRAW32_MAX_SLOT)
  path     "prefix" tpe_lattice_suggest (at most LAT_SUGGEST_MAX_SLOTS slots),
           "compact" sample -> compact -> score
  variant  "wave"   both mixtures of at most K_QBIG components (qlpdf),
           "block"  the above mixture past K_QBIG (qlpdf_block)
  rare     True: the history puts below and above together, so the best values
           lie in the tails and some value that beats everything in the first
           PREFIX candidates is first drawn after them (tpe_lattice_suggest
           must draw the rest); False ("settled"): no such value.

The histories are either natural (draws from the prior split by random losses
at gamma 0.25: T_WAVE trials -> 5 below / 315 above, T_BLOCK -> 17 / 4233) or
rare-winner (N_BELOW below observations tightly around the centre, the above
ones loosely around the same centre: the construction of
test_gpu_lattice.test_lattice_prefix_decision_equals_full_stream, see _rare).
The keys of the rare cases were chosen by a search over the replay for a late
winner with a wide margin; test_lattice_cases.py asserts every premise from
the table as it stands.

LEVELS are the launches of several jobs that the decision tests run: each
mixes rare-winner cases, settled ones and a job of at most PREFIX candidates.
"""
import math
from collections import namedtuple

import numpy as np

from hyperopt_amd import engine as E
from hyperopt_amd import _lib as L
from oracle import streams as S
from oracle import tpe_oracle as O
from tests import scale_cases as SC
from tests import stream_cases as STC

# the kernels' constants (csrc/tpe_quantized.hip, tpe_common.hpp; no export)
TILE = 4096          # kBS * kLatR: candidates of one sampler tile
K_LAT_LDS = 4096     # kLatLds: slots deduplicated in LDS
K_QBIG = 4096        # kQBig: components above which a value takes the whole block
PREFIX = TILE        # the smallest prefix tpe_lattice_suggest and the engine accept
N_FULL = 3 * TILE + 77
N_ODD = (1, 100, TILE, N_FULL)
BASE_ODD = 2 ** 33 + 12345   # an odd shard base past 2^32
GAMMA = 0.25
T_WAVE, T_BLOCK = 320, 4250
N_BELOW = 25
A_WAVE, A_BLOCK = 300, 4225  # above observations of the rare-winner histories
REDO = 8e-16         # the tie window of `mark`: |frac(t) - 1/2| <= REDO |t|

Case = namedtuple("Case", "name kind args below above key n_cand draw path variant rare")


def _key(i):
    return (0x1A771CE000000000 + 0x9E3779B97F4A7C15 * (i + 1)) & 0xFFFFFFFFFFFFFFFF


def _natural(kind, args, T, seed):
    rng = np.random.RandomState(seed)
    q = args[2]
    if kind == "quniform":
        v = rng.uniform(args[0], args[1], T)
    elif kind == "qloguniform":
        v = np.exp(rng.uniform(args[0], args[1], T))
    elif kind == "qnormal":
        v = rng.normal(args[0], args[1], T)
    else:
        v = np.exp(rng.normal(args[0], args[1], T))
    v = np.round(v / q) * q
    losses = np.random.RandomState(seed + 1).normal(size=T)
    return O.ap_split_trials(np.arange(T), v, np.arange(T), losses, GAMMA)


def _rare(kind, args, n_above, seed, centre, tight, loose, outliers=()):
    """below: N_BELOW observations at centre +- tight, above: n_above at
    centre +- loose (normal, in the fit's coordinate: log x for the log
    kinds), its oldest observations moved to `outliers` in the tails.  Far from
    the centre both mixtures are their priors alone and the score sits on the
    plateau of the two prior weights' ratio, every margin zero; the outliers
    -- wide components (sigma = the gap to the bulk) of almost no weight
    (linear forgetting: the oldest of 300 weighs 1 / 300) -- tilt that
    plateau by a few per cent of the above prior's mass, so the scores rise
    towards the rare end of each tail."""
    rng = np.random.RandomState(seed)
    q = args[2]
    b, a = rng.normal(centre, tight, N_BELOW), rng.normal(centre, loose, n_above)
    a[:len(outliers)] = outliers
    if "log" in kind:
        b, a = np.exp(b), np.exp(a)
    b, a = np.round(b / q) * q, np.round(a / q) * q
    if kind in ("quniform", "qloguniform"):
        lo, hi = (args[0], args[1]) if kind == "quniform" else (math.exp(args[0]),
                                                                  math.exp(args[1]))
        b, a = np.clip(b, lo, hi), np.clip(a, lo, hi)
    return b, a


def _wide_qu_history(T, seed):
    """quniform(0, 6000, 1): the below observations spread over both sides of
    slot K_LAT_LDS, so the drawn slots lie below and above it."""
    rng = np.random.RandomState(seed)
    v = np.round(rng.uniform(0.0, 6000.0, T))
    losses = np.random.RandomState(seed + 1).normal(size=T)
    return O.ap_split_trials(np.arange(T), v, np.arange(T), losses, GAMMA)


def _build():
    cases = []

    def add(name, kind, args, hist, draw, path, variant="wave", rare=False, key=None,
            n_cand=N_FULL):
        b, a = hist
        cases.append(Case(name, kind, tuple(float(x) for x in args), np.asarray(b, float),
                          np.asarray(a, float), _key(len(cases)) if key is None else key, n_cand,
                          draw, path, variant, rare))

    def nat(kind, args, variant="wave", seed=0):
        return _natural(kind, args, T_WAVE if variant == "wave" else T_BLOCK, 8100 + seed)

    # ---- the POW2 instantiation ---------------------------------------------------
    add("quniform(0,100,1)", "quniform", (0, 100, 1), nat("quniform", (0, 100, 1)), "pow2",
        "prefix")
    add("quniform(-3,7,0.25)", "quniform", (-3, 7, 0.25), nat("quniform", (-3, 7, 0.25), seed=1),
        "pow2", "prefix")
    # ---- fp32 draws, general instantiation ----------------------------------------
    add("quniform(0,10,0.1)", "quniform", (0, 10, 0.1), nat("quniform", (0, 10, 0.1), seed=2),
        "gen32", "prefix")
    add("quniform(0,100,3)", "quniform", (0, 100, 3), nat("quniform", (0, 100, 3), seed=3),
        "gen32", "prefix")
    add("quniform(0,100,3)/block", "quniform", (0, 100, 3),
        nat("quniform", (0, 100, 3), "block", seed=4), "gen32", "prefix", "block")
    add("qnormal(0,10,3)", "qnormal", (0, 10, 3), nat("qnormal", (0, 10, 3), seed=5), "gen32",
        "prefix")
    add("qloguniform(0,4,3)", "qloguniform", (0, 4, 3), nat("qloguniform", (0, 4, 3), seed=6),
        "gen32", "prefix")
    # ---- fp64 draws ---------------------------------------------------------------
    b, a = nat("quniform", (0, 100, 1), seed=7)
    add("quniform(1e6,1e6+100,1)", "quniform", (1e6, 1e6 + 100, 1), (b + 1e6, a + 1e6), "gen64",
        "prefix")
    add("quniform(0,6000,1)", "quniform", (0, 6000, 1), _wide_qu_history(T_WAVE, 8120), "gen64",
        "compact")
    add("quniform(0,6000,1)/block", "quniform", (0, 6000, 1), _wide_qu_history(T_BLOCK, 8122),
        "gen64", "compact", "block")
    add("qlognormal(0,1,0.5)", "qlognormal", (0, 1, 0.5), nat("qlognormal", (0, 1, 0.5), seed=13),
        "gen64", "compact")
    add("qlognormal(0,1,0.5)/block", "qlognormal", (0, 1, 0.5),
        nat("qlognormal", (0, 1, 0.5), "block", seed=9), "gen64", "compact", "block")
    # ---- rare winners: one per family, plus an fp64 one and a block one --------------
    def rare(name, kind, args, n_above, seed, centre, tight, loose, outliers, draw, path,
             variant="wave", shift=0.0):
        b, a = _rare(kind, args, n_above, seed, centre, tight, loose, outliers)
        args = tuple(x + (shift if i < 2 else 0.0) for i, x in enumerate(args))
        add(name, kind, args, (b + shift, a + shift), draw, path, variant, True, RARE_KEYS[name])

    rare("rare:quniform(0,100,1)", "quniform", (0, 100, 1), A_WAVE, 8200, 50.0, 1.0, 10.0,
         (12.0, 88.0), "pow2", "prefix")
    rare("rare:quniform(0,100,1)/block", "quniform", (0, 100, 1), A_BLOCK, 8201, 50.0, 1.0, 6.0,
         (12.0, 88.0) * 4, "pow2", "prefix", "block")
    rare("rare:quniform(1e6,1e6+100,1)", "quniform", (0, 100, 1), A_WAVE, 8202, 50.0, 1.0, 10.0,
         (15.0, 85.0) * 2, "gen64", "prefix", shift=1e6)
    rare("rare:qloguniform(2,6,1)", "qloguniform", (2, 6, 1), A_WAVE, 8203, 4.0, 0.05, 0.4,
         (5.3,), "pow2", "prefix")
    rare("rare:qnormal(0,10,0.25)", "qnormal", (0, 10, 0.25), A_WAVE, 8204, 0.0, 0.3, 1.0,
         (-12.0, 12.0), "pow2", "prefix")
    rare("rare:qlognormal(3,0.5,1)", "qlognormal", (3, 0.5, 1), A_WAVE, 8205, 3.0, 0.03, 0.05,
         (4.5, 1.5), "pow2", "compact")
    return cases


# keys of the rare-winner cases (see the module docstring)
RARE_KEYS = {
    "rare:quniform(0,100,1)": 0x5EED0000,
    "rare:quniform(0,100,1)/block": 0x5EEDF778,
    "rare:quniform(1e6,1e6+100,1)": 0x5EEE1667,
    "rare:qloguniform(2,6,1)": 0x5EEE5445,
    "rare:qnormal(0,10,0.25)": 0x5EEED001,
    "rare:qlognormal(3,0.5,1)": 0x5EED1EEF,
}

CASES = _build()
IDS = [c.name for c in CASES]
BY_NAME = dict(zip(IDS, CASES))
RARE = [c for c in CASES if c.rare]
SETTLED = [c for c in CASES if not c.rare and c.path == "prefix"]
WIDE = [c for c in CASES if c.path == "compact" and not c.rare]


def case(name):
    return BY_NAME[name]


# launches of several jobs: (case name, n_cand)
LEVELS = {
    # every job on the POW2 instantiation
    "pow2": [("rare:quniform(0,100,1)", N_FULL), ("quniform(0,100,1)", N_FULL),
             ("rare:qnormal(0,10,0.25)", N_FULL), ("quniform(-3,7,0.25)", 100),
             ("rare:qloguniform(2,6,1)", N_FULL)],
    # a non-pow2 q moves the pow2 jobs onto the general instantiation
    "gen32": [("rare:quniform(0,100,1)", N_FULL), ("quniform(0,100,3)", N_FULL),
              ("rare:qnormal(0,10,0.25)", N_FULL), ("quniform(-3,7,0.25)", 100),
              ("rare:qloguniform(2,6,1)", N_FULL), ("quniform(0,10,0.1)", TILE)],
    # fp32 and fp64 draws side by side; a lattice past LAT_SUGGEST_MAX_SLOTS
    "gen64": [("rare:quniform(1e6,1e6+100,1)", N_FULL), ("quniform(0,100,1)", N_FULL),
              ("rare:qlognormal(3,0.5,1)", N_FULL), ("qloguniform(0,4,3)", 1),
              ("quniform(1e6,1e6+100,1)", N_FULL)],
    # block-variant jobs beside wave-variant ones
    "block": [("rare:quniform(0,100,1)/block", N_FULL), ("quniform(0,100,3)/block", N_FULL),
              ("rare:quniform(0,100,1)", N_FULL), ("quniform(0,100,1)", 100)],
}


def level(name):
    return [BY_NAME[n]._replace(n_cand=k) for n, k in LEVELS[name]]


# ---------------------------------------------------------------------------
# what the engine derives from a case
# ---------------------------------------------------------------------------
def spec(c):
    """(family, prior_mu, prior_sigma, transform, low, high, q)."""
    return O.posterior_spec(c.kind, c.args)


def fits(c):
    """The oracle's (w, mu, sigma) of the below and the above mixture."""
    fam, pmu, psig, tf, low, high, q = spec(c)
    return tuple(O.adaptive_parzen_normal(tf(np.asarray(o, float)), 1.0, pmu, psig)
                 for o in (c.below, c.above))


def lattice(c):
    """(kmin, slots) as Engine plans it (engine._lattice_range)."""
    w = E.LabelWork("q", c.kind, c.args, c.below, c.above, n_cand=c.n_cand, key=c.key)
    kmin, kmax = E._lattice_range(w, E.posterior_params(c.kind, c.args))
    return kmin, kmax - kmin + 1


def is_pow2(q):
    m, e = math.frexp(q)
    return m == 0.5 and -100 < e < 100


def route(c):
    """(draw, path, variant) by the engine's and the kernels' rules at
    precision 32: engine.py's DRAW32 flag, lattice_pow2, _score_lat's choice
    and qlpdf_big."""
    kmin, n = lattice(c)
    draw32 = max(abs(kmin), abs(kmin + n - 1)) <= E.DRAW32_MAX_SLOT
    draw = "gen64" if not draw32 else ("pow2" if is_pow2(c.args[2]) and n <= K_LAT_LDS
                                       else "gen32")
    path = "prefix" if n <= E.LAT_SUGGEST_MAX_SLOTS else "compact"
    fb, fa = fits(c)
    variant = "block" if max(fb[0].size, fa[0].size) > K_QBIG else "wave"
    return draw, path, variant


def job_flags(c, draw=None):
    low = spec(c)[4]
    f = L.F_QUANT | ((L.F_LOW | L.F_HIGH) if low is not None else 0)
    return f | (L.F_DRAW32 if (draw or c.draw) != "gen64" else 0)


def oracle_scores(c, values):
    with np.errstate(all="ignore"):
        r = O.continuous_label_scores(c.kind, c.args, c.below, c.above,
                                      np.asarray(values, np.float64))
        return r["below_llik"] - r["above_llik"], r


def noise(c, values):
    """scale_cases.oracle_noise on a case's lattice values: the oracle's
    disagreement with itself under the label's power-of-two image."""
    sc = SC.Case("lattice:" + c.name, c.kind, c.args, c.below, c.above,
                 np.asarray(values, float), "self", None, None, None, None, c.key, None)
    return SC.oracle_noise(sc)


# ---------------------------------------------------------------------------
# the numpy replay of a case's stream
# ---------------------------------------------------------------------------
_Fam = namedtuple("_Fam", "family")


def replay(c, n=None, base=0, draw=None):
    """(k, ambiguous): lattice index rint(v / q) of candidates base .. base + n
    of the case's stream (fp32 or fp64 by `draw`), and the draws that
    stream_cases.quant_index marks ambiguous (within the replay's tolerance of
    a half-step)."""
    fam, pmu, psig, tf, low, high, q = spec(c)
    w, mu, sigma = fits(c)[0]
    cdf = np.cumsum(w) / np.sum(w)
    g = base + np.arange(c.n_cand if n is None else n, dtype=np.int64)
    if (draw or c.draw) == "gen64":
        rep = S.gmm_draw64(cdf, mu, sigma, c.key, g, low, high)
        tol = STC.tol64(rep, mu, sigma)
        return STC.quant_index(_Fam(fam), rep, q, tol, False)
    rep = S.gmm_draw32(cdf, mu, sigma, c.key, g, low, high)
    rep["y"] = rep["y"].astype(np.float32).astype(np.float64)  # the device's fp32 draw
    return STC.quant_index(_Fam(fam), rep, q, STC.tol32(rep, rep["y"]), True)


def premise(c, k, q=None, ok=None):
    """From a stream's lattice indices k (candidate order): dict with
    values / first / score of the distinct values, `winner` (np.argmax's
    candidate index), `margin` (winner's score minus the runner-up value's),
    `late` (values scoring strictly above the best of the first PREFIX
    candidates whose first occurrence is at or past PREFIX).  ok: draws to
    keep (the replay's unambiguous ones)."""
    q = c.args[2] if q is None else q
    idx = np.arange(k.size) if ok is None else np.flatnonzero(ok)
    u, f = np.unique(k[idx], return_index=True)
    f = idx[f]
    vals = u.astype(np.float64) * q
    s, r = oracle_scores(c, vals)
    assert not np.any(np.isnan(s)), (c.name, vals[np.isnan(s)])
    order = np.lexsort((f, -s))           # best score first, earliest first among equals
    top = order[0]
    margin = float(s[top] - s[order[1]]) if order.size > 1 else np.inf
    early = f < PREFIX
    best_early = s[early].max() if early.any() else -np.inf
    late = (~early) & (s > best_early)
    lp = max(abs(r["below_llik"][top]), abs(r["above_llik"][top]))
    return dict(values=vals, first=f, score=s, winner=int(f[top]), margin=margin,
                late=vals[late], late_margin=float((s[late] - best_early).max()) if late.any()
                else 0.0, lpdf=float(lp))


_premise = {}


def replay_premise(c):
    """premise() of the case's replayed stream without its ambiguous draws
    (cached by name and candidate count); `ambiguous` is their number."""
    k_ = (c.name, c.n_cand)
    if k_ not in _premise:
        k, amb = replay(c)
        p = premise(c, k, ok=~amb)
        p["ambiguous"] = int(amb.sum())
        p["slots"] = np.unique(k[~amb]) - lattice(c)[0]
        _premise[k_] = p
    return _premise[k_]


def fair_margin(p):
    """The margin above which "index == np.argmax of the oracle's scores" is a
    fair exact assertion: the kernels' log-masses are pinned to the oracle's
    within 1e-8 (1 + |lpdf|) per side (test_gpu_mixture), so two scores can
    move against each other by four times that."""
    return 4e-8 * (1.0 + p["lpdf"])


# ---------------------------------------------------------------------------
# explicit mixtures: rounding ties and the clamp
# ---------------------------------------------------------------------------
TIE_Q = (0.1, 0.3, 3.0, 1e-3, 0.25)
TIE_REL_SIGMA = 1e-12
TIE_TIGHT = 2e-16    # fp64 stream: every draw is its mean or a double next to it
TIE_KEY = 0x71E5EED


def tie_mixture(q, rel=TIE_REL_SIGMA):
    """(mu, sigma, w, kmin, slots): components at (k + 1/2) q for lattice
    indices k at which that product is a float (so the fp32 stream's draws sit
    on the tie exactly; in fp64 (k + 1/2) * q rounds to the double next to
    it), sigmas of rel |mu|.  At TIE_REL_SIGMA a few fp64 draws in 10^4 fall
    into the redo window; at TIE_TIGHT nearly all do, and for some q (see
    differ_count) the multiplication alone would round many of them to the
    other neighbour."""
    ks = [k for k in range(0, 4000) if float(np.float32((k + 0.5) * q)) == (k + 0.5) * q][:12]
    assert len(ks) >= 4, q
    ks = np.asarray(ks + [-k - 1 for k in ks], np.int64)
    mu = np.sort((ks + 0.5) * q)
    return mu, rel * np.abs(mu), np.ones(mu.size), int(ks.min()) - 2, \
        int(ks.max() - ks.min()) + 6


def tie_stream(q, key, n, fp32, base=0, rel=TIE_REL_SIGMA):
    """The replayed unquantized draws of tie_mixture(q, rel) (as doubles)."""
    mu, sigma, w, _, _ = tie_mixture(q, rel)
    cdf = np.cumsum(w) / w.sum()
    g = base + np.arange(n, dtype=np.int64)
    if fp32:
        y = S.gmm_draw32(cdf, mu, sigma, key, g)["y"]
        return y.astype(np.float32).astype(np.float64)
    return S.gmm_draw64(cdf, mu, sigma, key, g)["y"]


def redo_count(v, q):
    """Draws that take `mark`'s redo branch: t = v * (1 / q) within REDO |t|
    of a half-integer."""
    t = np.asarray(v, np.float64) * (1.0 / q)
    return int(np.sum(np.abs(np.abs(t - np.rint(t)) - 0.5) <= REDO * np.abs(t)))


def differ_count(v, q):
    """Draws that v * (1 / q) alone puts on another lattice index than
    rint(v / q): what the redo branch is there for."""
    v = np.asarray(v, np.float64)
    return int(np.sum(np.rint(v * (1.0 / q)) != np.rint(v / q)))


TIE_DIFFER_Q = (0.1, 3.0)   # q at which the tight fp64 stream holds such draws


CLAMP_LOW, CLAMP_HIGH, CLAMP_Q = 0.0, 10.0, 3.0


CLAMP_KMIN, CLAMP_SLOTS = -1, 6   # slots -1 .. 4: the brackets and bins 0 .. 3
CLAMP_W_IN = 1.2e-6               # ~1e-4 per candidate over its 256 attempts


def clamp_mixture(side, inside=False):
    """(mu, sigma, w) of the below mixture: every component ~40 sigma outside
    [CLAMP_LOW, CLAMP_HIGH] on one side, so every attempt is rejected and the
    last one clamped to the bound on that side; inside: one more component
    within the bounds whose weight makes about one candidate in 10^4 land
    inside."""
    mu = np.array([-41.0, -40.0, -39.0]) if side == "low" else np.array([49.0, 50.0, 51.0])
    sigma, w = np.ones(3), np.ones(3)
    if inside:
        mu, sigma, w = np.append(mu, 4.4), np.append(sigma, 1.5), np.append(w, CLAMP_W_IN)
        o = np.argsort(mu)
        mu, sigma, w = mu[o], sigma[o], w[o]
    return mu, sigma, w


def clamp_slot(side):
    """Lattice index of the bin that holds the bound the clamp lands on (low
    itself, or the last double below high)."""
    b = CLAMP_LOW if side == "low" else float(np.nextafter(CLAMP_HIGH, -np.inf))
    return int(np.rint(b / CLAMP_Q))


def clamp_above(side, inside_wins):
    """(mu, sigma, w) of the above mixture: one component that leaves the
    inside values scoring above the clamp's slot, or below it."""
    if inside_wins:
        m = 0.0 if side == "low" else 10.0
    else:
        m = 8.0 if side == "low" else 2.0
    return np.array([m]), np.array([2.0]), np.ones(1)


def clamp_stream(side, key, n, fp32, inside=False, base=0):
    """(lattice index of the replayed draws, clamped flags)."""
    mu, sigma, w = clamp_mixture(side, inside)
    cdf = np.cumsum(w) / w.sum()
    g = base + np.arange(n, dtype=np.int64)
    rep = (S.gmm_draw32 if fp32 else S.gmm_draw64)(cdf, mu, sigma, key, g, CLAMP_LOW, CLAMP_HIGH)
    y = rep["y"].astype(np.float32).astype(np.float64) if fp32 else rep["y"]
    return np.rint(y / CLAMP_Q).astype(np.int64), rep["clamped"]


def clamp_scores(side, inside_wins, inside=True):
    """The oracle's below - above log-mass of slots CLAMP_KMIN .. (NaN on the
    brackets)."""
    vals = (CLAMP_KMIN + np.arange(CLAMP_SLOTS)) * CLAMP_Q
    mb, sb, wb = clamp_mixture(side, inside)
    ma, sa, wa = clamp_above(side, inside_wins)
    with np.errstate(all="ignore"):
        return O.gmm1_lpdf(vals, wb / wb.sum(), mb, sb, CLAMP_LOW, CLAMP_HIGH, CLAMP_Q) - \
            O.gmm1_lpdf(vals, wa / wa.sum(), ma, sa, CLAMP_LOW, CLAMP_HIGH, CLAMP_Q)


# keys of the inside sub-cases: the first inside draw falls past the prefix
CLAMP_KEYS = {("low", True): 0xC1D3232, ("low", False): 0xC1B9919, ("high", True): 0xC1A0000,
              ("high", False): 0xC1A0000}
