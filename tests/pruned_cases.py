"""Case table shared by tests/test_pruned_cases.py (the oracle alone, no GPU)
and tests/test_gpu_pruned64_stages.py (the pruned exact fp64 scorer,
csrc/tpe_pruned64.hip, and the dense fp64 kernel beside it).

  sizes      the four continuous kinds x above mixtures of N_ABOVE observations
             (nc = n + 1 components around the 64-component staging chunk and
             the 256-component plan tile) x below mixtures of N_BELOW
  cluster    test_gpu_table_cells._cluster: duplicates, a cluster in 1 % of the
             range, isolated points (ties among the sorted means); both roles
  spread     uniform, 2000 above observations spread evenly over the range:
             every sigma is range / 100, so a window holds about a fifth of
             the components
  threshold  normal(0, 1) / lognormal(0, 1): 25 below observations at 90 +
             1e-3 i, candidates 33.0, 33.1, ..., 39.0 -- inside the planned
             range, where the pruned sum runs through normal values, values
             below 2^-900, subnormals and exactly 0
  neighbours one uniform mixture (300 above / 25 below) and 4097 candidates

Every candidate set starts with two anchors beyond mu +- 8.7 sigma of every
below component (at the bounds of a bounded kind), so the clip of the planned
range to the injected candidates is inactive and the plan does not depend on
the rest of the set.  The longdouble reference (terms, lse) and the plan's
range and floors restated are here too; test_pruned_cases.py proves the
premises from the oracle's fit.
"""
from collections import namedtuple

import numpy as np

from oracle import tpe_oracle as O
from tests.band_util import CONT, LGMM
from tests.table_util import DRAW_Z64, TAU_EXACT

LD = np.longdouble

# the kernel's constants (csrc/tpe_pruned64.hip; no export)
TILE = 2048            # kP64N: candidates a block sorts together
RUN = 64               # a wave scores runs of 64 sorted candidates
SLOW_BELOW = 2.0 ** -900   # a pruned sum below this is redone over every component
EXP_CUT = -745.2       # exp_neg64 returns 0 below it
MAX_COMP, MAX_CAND = 2001, 4100   # the size cap of a case

N_ABOVE = (0, 1, 63, 64, 127, 255, 256, 512)
N_BELOW = (0, 3, 25)
N_DRAWS = 192          # candidates drawn from the prior in every set
SWEEP = np.round(np.arange(33.0, 39.05, 0.1), 1)
THRESHOLD = [("normal", (0.0, 1.0)), ("lognormal", (0.0, 1.0))]
SPLITS = (1, 63, 64, 65, 2047, 2048, 2049)
N_NEIGHBOURS = 4097

Case = namedtuple("Case", "name kind args below above")


def draw(rng, kind, args, n):
    """n values of the kind's prior (unclipped for the normal kinds)."""
    if kind in ("uniform", "loguniform"):
        v = rng.uniform(args[0], args[1], n)
    else:
        v = rng.normal(args[0], args[1], n)
    return np.exp(v) if kind in LGMM else v


def to_x(kind, y):
    """A candidate value whose scoring coordinate is (the double next to) y."""
    y = np.asarray(y, np.float64)
    return np.exp(y) if kind in LGMM else y


def to_y(kind, x):
    """The scoring coordinate as the engine's host side forms it."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return np.log(x) if kind in LGMM else x


def _cases():
    from tests.test_gpu_table_cells import _cluster
    out = []
    for ki, (kind, args) in enumerate(CONT):
        for nb in N_BELOW:
            for na in N_ABOVE:
                rng = np.random.RandomState(8100 + 1000 * ki + 10 * na + nb)
                out.append(Case("sizes-%s-%d-%d" % (kind, nb, na), kind, args,
                                draw(rng, kind, args, nb), draw(rng, kind, args, na)))
        big, small = _cluster(kind, args)
        out.append(Case("cluster-%s" % kind, kind, args, small, big))
        out.append(Case("cluster-swapped-%s" % kind, kind, args, big, small))
    kind, args = CONT[0]
    rng = np.random.RandomState(8900)
    out.append(Case("spread-uniform-2000", kind, args, draw(rng, kind, args, 25),
                    np.linspace(args[0], args[1], 2002)[1:-1][rng.permutation(2000)]))
    for kind, args in THRESHOLD:
        rng = np.random.RandomState(8950)
        below = to_x(kind, 90.0 + 1e-3 * np.arange(25))
        out.append(Case("threshold-%s" % kind, kind, args, below, draw(rng, kind, args, 30)))
    rng = np.random.RandomState(8990)
    kind, args = CONT[0]
    out.append(Case("neighbours", kind, args, draw(rng, kind, args, 25),
                    draw(rng, kind, args, 300)))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
STAGED = [c.name for c in CASES if not c.name.startswith(("threshold", "neighbours"))]


def case(name):
    return BY_NAME[name]


# ---------------------------------------------------------------------------
# the oracle's fit, as coefficient rows {mu, 1 / sigma, log-coefficient}
# ---------------------------------------------------------------------------
def fit(c, side):
    """(w, mu, sigma) of the case's below / above mixture (the oracle's)."""
    fam, pmu, psig, tf, low, high, q = O.posterior_spec(c.kind, c.args)
    obs = tf(np.asarray(c.below if side == "below" else c.above, np.float64))
    return O.adaptive_parzen_normal(obs, 1.0, pmu, psig)


def oracle_coef(c, side):
    """[nc, 3] rows {mu, 1 / sigma, lc} in fp64: lc = log(w / (sigma sqrt(2
    pi)) / p_accept) for GMM1 (gmm1_lpdf), log w - log(sigma sqrt(2 pi)) for
    LGMM1 in y = log x (lgmm1_lpdf's unquantized branch ignores p_accept)."""
    fam, pmu, psig, tf, low, high, q = O.posterior_spec(c.kind, c.args)
    w, mu, sigma = fit(c, side)
    p_acc = O._p_accept(w, mu, sigma, low, high) if fam == "GMM1" else 1
    lc = np.log(w / np.sqrt(2 * np.pi * sigma ** 2) / p_acc)
    return np.stack([mu, 1.0 / sigma, lc], axis=1)


# ---------------------------------------------------------------------------
# the longdouble reference
# ---------------------------------------------------------------------------
def terms(coef, y):
    """[candidate, component] log-terms lc - 0.5 ((y - mu) inv)^2, longdouble."""
    mu, inv, lc = (np.asarray(coef[:, i], np.float64).astype(LD) for i in range(3))
    t = (np.asarray(y).astype(LD)[:, None] - mu) * inv
    return lc - LD(0.5) * t * t


def lse(v):
    """log sum exp over the last axis, longdouble."""
    m = v.max(axis=1)
    return np.log(np.exp(v - m[:, None]).sum(axis=1)) + m


def reference(kind, coef, x):
    """L(y) of every component, minus y for the LGMM1 kinds (lognormal_lpdf's
    -log x); y = log x in longdouble there."""
    x = np.asarray(x, np.float64)
    y = np.log(x.astype(LD)) if kind in LGMM else x.astype(LD)
    out = lse(terms(coef, y))
    return out - y if kind in LGMM else out


def fast_sum(coef, y):
    """The pruned kernel's fp64 sum of every component at y: sum_j exp(v_j -
    max lc), exp 0 below EXP_CUT (a superset of the window and wide list)."""
    coef = np.asarray(coef, np.float64)
    y = np.asarray(y, np.float64)
    t = (y[:, None] - coef[:, 0]) * coef[:, 1]
    v = -0.5 * t * t + (coef[:, 2] - coef[:, 2].max())
    with np.errstate(under="ignore"):
        e = np.where(v < EXP_CUT, 0.0, np.exp(v))
    return e.sum(axis=1)


# ---------------------------------------------------------------------------
# the plan's range and floors, restated (plan_range, tpe_table.hip)
# ---------------------------------------------------------------------------
def plan_range(kind, args, mu_b, sigma_b, x_cand):
    """(lo, hi): min / max of mu -+ 8.7 sigma over the below components,
    clipped to the finite injected candidates' range in the scoring coordinate
    and to [low, high] where the kind is bounded."""
    low, high = O.posterior_spec(kind, args)[4:6]
    a, b = np.min(mu_b - DRAW_Z64 * sigma_b), np.max(mu_b + DRAW_Z64 * sigma_b)
    y = to_y(kind, x_cand)
    y = y[np.isfinite(y)]
    a, b = max(a, y.min()), min(b, y.max())
    if low is not None:
        a, b = max(a, low), min(b, high)
    assert np.isfinite(a) and np.isfinite(b) and b >= a
    return a, b


def floor_of(coef, prior_pos, lo, hi):
    """T = lc_prior - 0.5 far^2 - (log nc + 40)."""
    mu, inv, lc = coef[prior_pos, :3]
    far = max(abs(lo - mu), abs(hi - mu)) * inv
    return lc - 0.5 * far * far - (np.log(float(coef.shape[0])) + TAU_EXACT)


# ---------------------------------------------------------------------------
# candidates
# ---------------------------------------------------------------------------
def anchors(c):
    """Two candidates beyond mu +- 8.7 sigma of every below component in the
    scoring coordinate: the bounds of a bounded kind (for loguniform the
    doubles whose logs are at or beyond them), else 9 prior sigmas past the
    extreme means (no sigma exceeds the prior's)."""
    fam, pmu, psig, tf, low, high, q = O.posterior_spec(c.kind, c.args)
    if low is not None:
        a, b = to_x(c.kind, low), to_x(c.kind, high)
        while to_y(c.kind, a) > low:
            a = np.nextafter(a, -np.inf)
        while to_y(c.kind, b) < high:
            b = np.nextafter(b, np.inf)
        return np.array([a, b], np.float64)
    w, mu, sigma = fit(c, "below")
    return to_x(c.kind, np.array([mu.min() - 9.0 * psig, mu.max() + 9.0 * psig]))


def draws(c, n=N_DRAWS, seed=0):
    return draw(np.random.RandomState(9200 + seed + len(c.name)), c.kind, c.args, n)


def base_candidates(c):
    """The first run's set: the anchors, then draws from the prior (for the
    threshold cases the sweep instead)."""
    if c.name.startswith("threshold"):
        return np.concatenate([anchors(c), to_x(c.kind, SWEEP)])
    return np.concatenate([anchors(c), draws(c)])


def _both(v):
    v = np.asarray(v, np.float64)
    return np.concatenate([np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)])


def select(wide, nc):
    """The components whose window edges are injected: first, last, each side
    of (at most 8) wide components, 16 spread evenly."""
    w = np.flatnonzero(wide)[:8]
    k = np.concatenate([[0, nc - 1], w - 1, w + 1, np.linspace(0, nc - 1, 16).astype(np.int64)])
    return np.unique(k[(k >= 0) & (k < nc)]).astype(np.int64)


def edge_values(plan, lo, hi):
    """Scoring coordinates on the plan's window edges, from read-back arrays:
    ``plan`` is [(coef, reach_hi, reach_lo, wide flags)] of the two mixtures.
    reach_hi[k], reach_lo[k] and the doubles next to each, mu_k, for the
    selected k; lo, hi and their neighbours; all of these twice; one edge (lo
    where every component is wide) 64 times and one mean 2048 times."""
    vals, rep = [_both([lo, hi])], []
    for coef, rh, rl, wide in plan:
        k = select(wide, coef.shape[0])
        e = np.concatenate([rh[k], rl[k]])
        e = e[np.isfinite(e)]
        vals += [_both(e), coef[k, 0]]
        rep.append((e[e.size // 2] if e.size else lo, coef[k[k.size // 2], 0]))
    v = np.concatenate(vals)
    run, tile = rep[-1][0], rep[0][1]
    return np.concatenate([v, v, np.full(RUN, run), np.full(TILE, tile)])


def edge_candidates(c, plan, lo, hi):
    """The second run's set: anchors, then the edge values and the base
    draws under a fixed permutation (ties land in both tiles)."""
    rest = np.concatenate([to_x(c.kind, edge_values(plan, lo, hi)), base_candidates(c)[2:]])
    rest = rest[np.random.RandomState(9300).permutation(rest.size)]
    out = np.concatenate([anchors(c), rest])
    assert out.size <= MAX_CAND, out.size
    return out


def specials(kind):
    """Candidates without a finite scoring coordinate, or at its ends."""
    s = [np.inf, -np.inf, np.nan]
    if kind in LGMM:
        s += [0.0, -1.5, 5e-324, np.finfo(np.float64).max]
    return np.array(s, np.float64)


def neighbour_list():
    """4097 values of the neighbours case: draws with 200 exact duplicates."""
    c = case("neighbours")
    rng = np.random.RandomState(9400)
    v = draw(rng, c.kind, c.args, N_NEIGHBOURS - 200)
    v = np.concatenate([v, v[rng.randint(0, v.size, 200)]])
    return v[rng.permutation(v.size)]
