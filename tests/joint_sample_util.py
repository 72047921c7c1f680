"""The joint draw rule (hyperopt_amd/joint.py "Drawing") replayed
in plain numpy, for the tests.

Built on the pinned stream primitives of ``oracle/streams.py`` (``draw_words``,
``component_cdf``, ``normal_f64``, ``categorical_of_word``) and on the host
functions of ``hyperopt_amd/joint.py`` that describe a set (``label_models``,
``forgetting_weights``, ``bandwidths``, ``set_rows``); it holds no code of the
kernel.  ``replay_set`` takes a set as arrays, so a test can hand-write one;
``replay`` builds the below set of a history the way the device path does.

Shared by tests/test_joint_sample_host.py (the replay alone, no GPU) and
tests/test_gpu_joint_sample.py (the kernel against it), with the comparison
rules of tests/stream_cases.py for fp64 draws.
"""
import numpy as np

from hyperopt_amd import _lib as L
from hyperopt_amd import joint as J
from hyperopt_amd import tpe
from oracle import streams as S
from tests.stream_cases import CAP64, RTOL64

JOIN = J.STREAM_JOINT  # the stream word, 0x4A4F494E (asserted in test_joint_sample_host.py)
EPS = 1e-12


def model(kind, is_log=False, bounded=False, lo=0.0, hi=0.0, q=0.0, mu=0.0, sigma=1.0, p=None,
          col=0, label=None):
    """A hand-written ``joint.LabelModel`` (kind: "cont", "quant" or "cat")."""
    m = J.LabelModel()
    m.kind = {"cont": L.JOINT_CONT, "quant": L.JOINT_QUANT, "cat": L.JOINT_CAT}[kind]
    m.label, m.col = label, col
    m.is_log, m.bounded = bool(is_log), bool(bounded)
    m.lo, m.hi, m.q, m.mu, m.sigma = float(lo), float(hi), float(q), float(mu), float(sigma)
    m.p = None if p is None else np.asarray(p, np.float64)
    m.n_cat = 0 if p is None else int(m.p.size)
    m.offset = 0
    return m


def _continuous(m, mu, sigma, key, g):
    """Attempts a = 0, 1, ... at (g, a, JOIN): t = mu + sigma normal_f64(y, z, w),
    accepted when lo <= t < hi (always, unbounded); clamped after 256."""
    n = g.size
    t, z = np.zeros(n), np.zeros(n)
    attempts = np.zeros(n, np.int64)
    near = np.full(n, np.inf)
    todo = np.arange(n)
    for a in range(S.MAX_ATTEMPTS):
        r = S.draw_words(key, g[todo], a, JOIN)
        zz = S.normal_f64(r[:, 1], r[:, 2], r[:, 3])
        tt = mu[todo] + sigma[todo] * zz
        t[todo], z[todo], attempts[todo] = tt, zz, a + 1
        if not m.bounded:
            todo = todo[:0]
            break
        unit = np.abs(mu[todo]) + sigma[todo] * np.maximum(1.0, np.abs(zz))
        near[todo] = np.minimum(near[todo],
                                np.minimum(np.abs(tt - m.lo), np.abs(tt - m.hi)) / unit)
        todo = todo[~((m.lo <= tt) & (tt < m.hi))]
        if todo.size == 0:
            break
    clamped = np.zeros(n, bool)
    clamped[todo] = True
    tc = t[todo]
    tc = np.where(tc < m.lo, m.lo, tc)
    tc = np.where(~(tc < m.hi), np.nextafter(m.hi, -np.inf), tc)
    t[todo] = tc
    raw = np.exp(t) if m.is_log else t.copy()
    v = np.rint(raw / m.q) * m.q if m.kind == L.JOINT_QUANT else raw.copy()
    return dict(v=v, raw=raw, t=t, z=z, attempts=attempts, clamped=clamped, near=near, mu=mu,
                sigma=sigma)


def _discrete(m, cat, prior, key, g, one_plus_a):
    """Attempt 0 only: a trial component keeps its category when
    x 2^-32 (1 + a) < 1, else word y draws from the prior probabilities; the
    prior component draws with word x."""
    r = S.draw_words(key, g, 0, JOIN)
    cp = np.cumsum(m.p)
    keep = r[:, 0].astype(np.float64) * 2.0 ** -32 * float(one_plus_a) < 1.0
    v = np.where(prior, S.categorical_of_word(cp, r[:, 0]),
                 np.where(keep, cat, S.categorical_of_word(cp, r[:, 1])))
    n = g.size
    return dict(v=v.astype(np.float64), raw=v.astype(np.float64), t=None, z=np.zeros(n),
                attempts=np.ones(n, np.int64), clamped=np.zeros(n, bool),
                near=np.full(n, np.inf), kept=keep & ~prior)


def replay_set(models, mu, sig, cdf, keys, comp_key, one_plus_a, g):
    """Rows ``g`` drawn from a set given as arrays: ``mu`` (D, n) the trial
    components' means in the fit coordinate (the category for a discrete
    label), ``sig`` (D,) their bandwidths, ``cdf`` (n + 1,) the running sum of
    the weights with the prior last, ``keys`` the D label keys.
    Returns (comp, [per label dict(v, raw, z, attempts, clamped, near, ...)])."""
    g = np.atleast_1d(np.asarray(g, np.int64))
    cdf = np.asarray(cdf, np.float64)
    n = cdf.size - 1
    mu = np.asarray(mu, np.float64).reshape(len(models), n)
    comp = S.component_cdf(cdf, S.draw_words(comp_key, g, 0, JOIN)[:, 0])
    prior = comp == n
    ci = np.minimum(comp, max(n - 1, 0))
    out = []
    for d, m in enumerate(models):
        own = mu[d][ci] if n else np.zeros(g.size)
        if m.kind == L.JOINT_CAT:
            out.append(_discrete(m, own, prior, keys[d], g, one_plus_a))
        else:
            out.append(_continuous(m, np.where(prior, m.mu, own),
                                   np.where(prior, m.sigma, float(sig[d])), keys[d], g))
    return comp, out


def below_set(domain, hist, prior_weight=1.0, gamma=0.25, linear_forgetting=25,
              bandwidth=J.BANDWIDTH):
    """(models, mu (D, n), sig (D,), cdf) of the history's below set."""
    models = J.label_models(domain)
    cols = [m.col for m in models]
    isb = tpe.split_masks(hist, gamma)[0] if hist.tids.size else np.zeros(0, bool)
    rows = J.set_rows(hist, isb, cols)
    n = rows.size
    mu = np.zeros((len(models), n))
    for d, m in enumerate(models):
        obs = np.asarray(hist.vals)[rows, m.col] if n else np.zeros(0)
        if m.kind == L.JOINT_CAT:
            mu[d] = np.rint(obs) - m.offset
        else:
            mu[d] = np.log(np.maximum(obs, EPS)) if m.is_log else obs
    cdf = np.cumsum(np.concatenate([J.forgetting_weights(n, linear_forgetting),
                                    [float(prior_weight)]]))
    return models, mu, J.bandwidths(models, n, bandwidth), cdf


def replay(domain, hist, seed, g, prior_weight=1.0, gamma=0.25, linear_forgetting=25,
           bandwidth=J.BANDWIDTH, cat_smoothing=J.CAT_SMOOTHING):
    """Rows ``g`` of ``Pool.sample(..., joint=True)``'s joint labels:
    (models, comp, per-label dicts)."""
    models, mu, sig, cdf = below_set(domain, hist, prior_weight, gamma, linear_forgetting,
                                     bandwidth)
    keys = [tpe.label_key(seed, m.label) for m in models]
    comp, out = replay_set(models, mu, sig, cdf, keys, J.component_key(seed),
                           1.0 + float(cat_smoothing), g)
    return models, comp, out


# -- comparison rules (tests/stream_cases.py's, for this stream) -----------------
def tol_t(rep):
    """RTOL64 of |mu| + sigma max(1, |z|), in the fit coordinate."""
    return RTOL64 * (np.abs(rep["mu"]) + rep["sigma"] * np.maximum(1.0, np.abs(rep["z"])))


def tol_raw(m, rep):
    """The tolerance on the unquantized stored value: tol_t, carried through
    exp as a relative error for a log kind, plus an ulp of each side's exp."""
    if not m.is_log:
        return tol_t(rep)
    return rep["raw"] * (np.expm1(tol_t(rep)) + 4.0 * 2.0 ** -52)


def skipped(m, rep):
    """Rows the comparison leaves out: an attempt within RTOL64 of a bound
    (either side may accept it), and for a quantized label a value whose
    x / q lies within the tolerance of a half-integer."""
    skip = rep["near"] <= RTOL64
    if m.kind == L.JOINT_QUANT:
        s = rep["raw"] / m.q
        half = np.abs(np.abs(s - np.floor(s)) - 0.5) * m.q
        skip = skip | (half <= tol_raw(m, rep) + 4.0 * np.spacing(np.abs(rep["raw"])))
    return skip


def compare(m, rep, got):
    """Assert the device's column ``got`` against the replay of one label;
    returns (worst err / tol over the compared continuous rows, rows left
    out)."""
    got = np.asarray(got, np.float64)
    if m.kind == L.JOINT_CAT:
        np.testing.assert_array_equal(got, rep["v"])
        return 0.0, 0
    skip = skipped(m, rep)
    assert int(skip.sum()) <= CAP64, "%d ambiguous rows" % int(skip.sum())
    use = ~skip
    cl = use & rep["clamped"]
    if m.kind == L.JOINT_QUANT:
        np.testing.assert_array_equal(got[use], rep["v"][use])
        return 0.0, int(skip.sum())
    free = use
    if not m.is_log:  # a clamped draw is a bound: exact (a log kind's goes through exp)
        np.testing.assert_array_equal(got[cl], rep["v"][cl])
        free = use & ~rep["clamped"]
    ratio = np.abs(got[free] - rep["v"][free]) / tol_raw(m, rep)[free]
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, "err / tol = %.3g" % worst
    return worst, int(skip.sum())


# -- hand-written sets: the stage cases both files share -------------------------
STAGE = 64  # TPE_JOINT_SAMPLE_STAGE: component cdfs up to here are staged in LDS
ROWS = (1, 255, 256, 257, 300)
BASES = (0, 5, 2 ** 32 - 3, 2 ** 40 + 1)
COMPONENTS = (1, 2, 26, STAGE - 1, STAGE, STAGE + 1, 513)
SMOOTHING = (0.0, 0.5, 1.0)


def _key(i):
    return (0x2545F4914F6CDD1D * (i + 1) + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def _three():
    """A normal, a choice of 5 and a bounded quantized label."""
    return [model("cont", mu=1.0, sigma=2.0, col=0),
            model("cat", p=[0.1, 0.2, 0.3, 0.15, 0.25], col=1),
            model("quant", bounded=True, lo=0.0, hi=10.0, q=3.0, mu=5.0, sigma=10.0, col=2)]


def _filled(models, C, seed, bandwidth=0.3):
    """(mu, sig, cdf) of a set of C - 1 random trial components."""
    rng = np.random.RandomState(seed)
    n = C - 1
    mu = np.zeros((len(models), n))
    sig = np.zeros(len(models))
    for d, m in enumerate(models):
        if m.kind == L.JOINT_CAT:
            mu[d] = rng.randint(0, m.n_cat, n)
        elif m.bounded:
            mu[d] = rng.uniform(m.lo, m.hi, n)
            sig[d] = bandwidth * m.sigma
        else:
            mu[d] = m.mu + m.sigma * rng.normal(size=n)
            sig[d] = bandwidth * m.sigma
    return mu, sig, np.cumsum(np.concatenate([J.forgetting_weights(n, 25), [0.7]]))


def _case(name, models, mu, sig, cdf, n_rows, row_base, a=0.5, salt=0):
    return dict(name=name, models=models, mu=mu, sig=sig, cdf=cdf, n_rows=n_rows,
                row_base=row_base, one_plus_a=1.0 + a,
                keys=[_key(100 * salt + d) for d in range(len(models))],
                comp_key=_key(100 * salt + 99))


def many_labels(D):
    """D labels cycling through the kinds (the log kinds and an unbounded
    quantized one included)."""
    kinds = [lambda c: model("cont", mu=0.5, sigma=1.5, col=c),
             lambda c: model("cont", bounded=True, lo=-2.0, hi=3.0, mu=0.5, sigma=5.0, col=c),
             lambda c: model("cont", is_log=True, bounded=True, lo=-2.0, hi=0.0, mu=-1.0, sigma=2.0,
                             col=c),
             lambda c: model("cont", is_log=True, mu=-1.0, sigma=1.0, col=c),
             lambda c: model("quant", bounded=True, lo=0.0, hi=10.0, q=3.0, mu=5.0, sigma=10.0,
                             col=c),
             lambda c: model("quant", mu=0.0, sigma=10.0, q=2.0, col=c),
             lambda c: model("quant", is_log=True, mu=0.0, sigma=2.0, q=1.0, col=c),
             lambda c: model("cat", p=np.full(7, 1.0 / 7), col=c),
             lambda c: model("cat", p=[0.0, 0.4, 0.6], col=c)]
    return [kinds[d % len(kinds)](d) for d in range(D)]


def stage_cases():
    """The hand-written cases of the stage test, by name."""
    out = []
    for i, C in enumerate(COMPONENTS):  # the component count, both sides of the staging cap
        models = _three()
        mu, sig, cdf = _filled(models, C, 10 + i)
        out.append(_case("C%d" % C, models, mu, sig, cdf, 300, BASES[i % len(BASES)], salt=i))
    models = _three()
    mu, sig, cdf = _filled(models, 26, 7)
    for i, rows in enumerate(ROWS):  # the launch geometry and the high counter word
        for k, base in enumerate(BASES):
            out.append(_case("rows%d-base%d" % (rows, k), models, mu, sig, cdf, rows, base,
                             salt=20 + 4 * i + k))
    one = [model("cont", bounded=True, lo=4.0, hi=7.0, mu=5.5, sigma=3.0, col=0)]
    mu, sig, cdf = _filled(one, 26, 3)
    out.append(_case("D1", one, mu, sig, cdf, 300, 5, salt=50))
    big = many_labels(128)
    mu, sig, cdf = _filled(big, 26, 4)
    out.append(_case("D128", big, mu, sig, cdf, 257, 2 ** 32 - 3, salt=51))
    # bandwidth 5 on uniform(0, 1): a trial component accepts 1 / (5 sqrt(2 pi)) = 8 %
    wide = [model("cont", bounded=True, lo=0.0, hi=1.0, mu=0.5, sigma=1.0, col=0)]
    mu, _, cdf = _filled(wide, 26, 5)
    out.append(_case("bandwidth5", wide, mu, np.asarray([5.0]), cdf, 300, 0, salt=52))
    # components 100 sigma outside [0, 1] on either side: every attempt is rejected
    far = np.asarray([[2.0, -1.0, 2.0, -1.0]])
    out.append(_case("clamp", wide, far, np.asarray([0.01]), np.cumsum([1.0, 1.0, 1.0, 1.0, 1e-9]),
                     300, 0, salt=53))
    # smoothing 0 (a trial component always keeps its category), 0.5, 1; a
    # zero-probability option that only a component of its own can give
    cats = [model("cat", p=[0.0, 0.4, 0.6], col=0), model("cat", p=np.full(9, 1.0 / 9), col=1)]
    mu, sig, cdf = _filled(cats, 26, 6)
    mu[0, :3] = 0.0
    for i, a in enumerate(SMOOTHING):
        out.append(_case("smoothing%g" % a, cats, mu, sig, cdf, 300, 0, a=a, salt=60 + i))
    return out


def replay_case(c):
    g = c["row_base"] + np.arange(c["n_rows"], dtype=np.int64)
    return replay_set(c["models"], c["mu"], c["sig"], c["cdf"], c["keys"], c["comp_key"],
                      c["one_plus_a"], g)


# -- the distribution cases -------------------------------------------------------
DIST_SEED = 23
DIST_ROWS = 1 << 14


def truncated_mixture_cdf(m, mu, sig, cdf):
    """The cdf of a bounded continuous label's draws in the fit coordinate:
    the mixture of the components' normals truncated to [lo, hi)."""
    from scipy import stats
    w = np.diff(np.concatenate([[0.0], cdf])) / cdf[-1]
    mus = np.concatenate([mu, [m.mu]])
    sgs = np.concatenate([np.full(mu.size, sig), [m.sigma]])

    def F(t):
        t = np.asarray(t, np.float64)[..., None]
        a = stats.norm.cdf((m.lo - mus) / sgs)
        z = stats.norm.cdf((m.hi - mus) / sgs) - a
        return ((stats.norm.cdf((t - mus) / sgs) - a) / z * w).sum(-1)
    return F
