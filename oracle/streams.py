"""Plain-numpy replay of the library's random streams (no GPU).

Every draw the kernels make is a documented function of (label key, index,
attempt) through Philox4x32-10 (hyperopt_amd/csrc/tpe_common.hpp,
tpe_sample.hpp, tpe_categorical.hip, tpe_prior.hip, tpe_anneal.hip).  This
module restates those rules -- vectorised, 32-bit words carried in uint64
arrays and masked -- so a test can ask "is candidate g the documented function
of (key, g)?" instead of "does it look like the right distribution?".

Conventions: a counter is the four words {idx lo, idx hi, attempt, stream}, a
key the two words {key lo, key hi}.  Words are returned as uint64 arrays with
values < 2^32; indices may be any int64 (shard bases and trial ids >= 2^32
reach the high counter word).
"""
from __future__ import annotations

import numpy as np

SAMP = 0x53414D50  # candidate draws (attempt 0 of the fp32 stream, all fp64 attempts)
RETR = 0x52455452  # fp32 retries
PRIO = 0x5052494F  # prior draws
ANNL = 0x414E4E4C  # annealing: counter word 0 = the pick, 1 = the value

MAX_ATTEMPTS = 256               # fp64 attempts / fp32 attempts after the first
MAX_RETRY_CALLS = MAX_ATTEMPTS // 2
STAGE = 64                       # components staged with integer thresholds (fp32 stream)

PRIOR_UNIFORM, PRIOR_LOGUNIFORM, PRIOR_NORMAL, PRIOR_LOGNORMAL, PRIOR_RANDINT, \
    PRIOR_CATEGORICAL = range(6)

_M32 = np.uint64(0xFFFFFFFF)
_U = np.uint64


def _u64(x):
    return np.asarray(x).astype(np.uint64)


# ---------------------------------------------------------------------------
# Philox4x32 (Salmon et al., SC'11; Random123)
# ---------------------------------------------------------------------------
def philox4x32(counter4, key2, rounds=10):
    """counter4: (..., 4), key2: (..., 2) 32-bit words -> (..., 4) words."""
    c = _u64(counter4) & _M32
    k = _u64(key2) & _M32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(rounds):
        p0 = _U(0xD2511F53) * c0  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = _U(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> _U(32)) ^ c1 ^ k0, p1 & _M32,
                          (p0 >> _U(32)) ^ c3 ^ k1, p0 & _M32)
        k0 = (k0 + _U(0x9E3779B9)) & _M32
        k1 = (k1 + _U(0xBB67AE85)) & _M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def draw_words(key, idx, attempt, stream):
    """The four words of call (idx, attempt) of `stream` for label `key`:
    counter {idx lo, idx hi, attempt, stream}, key {key lo, key hi}."""
    idx = np.asarray(idx, dtype=np.int64).astype(np.uint64)
    att = _u64(attempt)
    idx, att = np.broadcast_arrays(idx, att)
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    ctr = np.stack([idx & _M32, idx >> _U(32), att & _M32,
                    np.full(idx.shape, stream, np.uint64)], axis=-1)
    return philox4x32(ctr, np.array([key & 0xFFFFFFFF, key >> 32], np.uint64))


# ---------------------------------------------------------------------------
# words -> uniforms and normals
# ---------------------------------------------------------------------------
def u01_f64(a, b):
    """[0, 1) with 53 random bits: 27 from a, 26 from b."""
    m = ((_u64(a) >> _U(5)) << _U(26)) | (_u64(b) >> _U(6))
    return m.astype(np.float64) * 2.0 ** -53


def u01_f32(a):
    """[0, 1) with 24 random bits (exact in fp32; returned as fp64)."""
    return (_u64(a) >> _U(8)).astype(np.float64) * 2.0 ** -24


def cos_turns32(c):
    """cos(2 pi c / 2^32) for a 32-bit word c, the angle reduced to an octant
    by integer arithmetic so the result keeps its relative accuracy next to
    the zeros of the cosine."""
    c = _u64(c)
    quad = (c >> _U(30)).astype(np.int64)
    rem = (c & _U((1 << 30) - 1)).astype(np.int64)
    upper = rem > (1 << 29)                     # past the middle of the quadrant
    a = np.where(upper, (1 << 30) - rem, rem).astype(np.float64) * (np.pi / 2 ** 31)
    ca = np.where(upper, np.sin(a), np.cos(a))  # cos / sin of the quadrant's own angle
    sa = np.where(upper, np.cos(a), np.sin(a))
    return np.choose(quad, [ca, -sa, -ca, sa])


def normal_f64(a, b, c):
    """Box-Muller, one of the pair: radius from u01_f64(a, b), angle from c."""
    u1 = 1.0 - u01_f64(a, b)  # (0, 1]
    return np.sqrt(-2.0 * np.log(u1)) * cos_turns32(c)


# ---------------------------------------------------------------------------
# component choice
# ---------------------------------------------------------------------------
def component_cdf(cdf, w):
    """The fp64 rule: the first k with cdf[k] > w * 2^-32 * cdf[-1]."""
    cdf = np.asarray(cdf, np.float64)
    u = _u64(w).astype(np.float64) * 2.0 ** -32 * cdf[-1]
    return np.minimum(np.searchsorted(cdf, u, side="right"), cdf.size - 1)


def thresholds(cdf):
    """thr[k] = ceil(cdf[k] / cdf[-1] * 2^32), saturated at 2^32 - 1."""
    cdf = np.asarray(cdf, np.float64)
    t = np.ceil(cdf / cdf[-1] * 4294967296.0)
    return np.where(t >= 4294967295.0, 4294967295.0, np.maximum(t, 0.0)).astype(np.uint64)


def component_thr(thr, w):
    """The threshold rule: the first k with w < thr[k] (the last one if none)."""
    return np.minimum(np.searchsorted(thr, _u64(w), side="right"), thr.size - 1)


def residual_thr(thr, k, w):
    """Upper residual of word w inside component k's word interval
    [thr[k-1], thr[k]): (thr[k] - w) / (thr[k] - thr[k-1]), in (0, 1]."""
    hi = thr[k].astype(np.float64)
    lo = np.where(k > 0, thr[np.maximum(k - 1, 0)], 0).astype(np.float64)
    width = hi - lo
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(width > 0, (hi - _u64(w).astype(np.float64)) / width, 0.0)


def residual_cdf(cdf, k, w):
    """The unstaged path's residual: (cdf[k] - u) / (cdf[k] - cdf[k-1])."""
    cdf = np.asarray(cdf, np.float64)
    u = _u64(w).astype(np.float64) * 2.0 ** -32 * cdf[-1]
    lo = np.where(k > 0, cdf[np.maximum(k - 1, 0)], 0.0)
    wk = cdf[k] - lo
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(wk > 0, (cdf[k] - u) / wk, 1.0)


def component_and_residual(cdf, w):
    """(component, upper residual) of word w as the fp32 stream takes them:
    integer thresholds for mixtures of at most STAGE components, the cdf
    itself for larger ones."""
    cdf = np.asarray(cdf, np.float64)
    if cdf.size <= STAGE:
        thr = thresholds(cdf)
        k = component_thr(thr, w)
        return k, residual_thr(thr, k, w)
    k = component_cdf(cdf, w)
    return k, residual_cdf(cdf, k, w)


# ---------------------------------------------------------------------------
# the fp64 candidate stream
# ---------------------------------------------------------------------------
def _bounds(low, high):
    return (-np.inf if low is None else float(low)), (np.inf if high is None else float(high))


def gmm_draw64(cdf, mu, sigma, key, g, low=None, high=None):
    """Candidates g of the fp64 stream, in the mixture's coordinate.

    Attempt a = 0..255 is the call at counter (g, a, SAMP): word x picks the
    component, words y, z, w feed the normal; the first attempt with
    low <= y < high is the draw; after 256 rejections the last attempt is
    clamped to low, or to nextafter(high, -inf).
    Returns dict(y, comp, z, attempts, clamped, near): `near` is the smallest
    distance of any attempt made to a bound, in units of that attempt's
    |mu_k| + sigma_k * max(1, |z|)."""
    cdf, mu, sigma = (np.asarray(a, np.float64) for a in (cdf, mu, sigma))
    g = np.atleast_1d(np.asarray(g, np.int64))
    lo, hi = _bounds(low, high)
    n = g.size
    y, comp, z = np.zeros(n), np.zeros(n, np.int64), np.zeros(n)
    attempts = np.zeros(n, np.int64)
    near = np.full(n, np.inf)
    todo = np.arange(n)
    for a in range(MAX_ATTEMPTS):
        r = draw_words(key, g[todo], a, SAMP)
        k = component_cdf(cdf, r[:, 0])
        zz = normal_f64(r[:, 1], r[:, 2], r[:, 3])
        yy = mu[k] + sigma[k] * zz
        y[todo], comp[todo], z[todo], attempts[todo] = yy, k, zz, a + 1
        unit = np.abs(mu[k]) + sigma[k] * np.maximum(1.0, np.abs(zz))
        near[todo] = np.minimum(near[todo],
                                np.minimum(np.abs(yy - lo), np.abs(yy - hi)) / unit)
        todo = todo[~((lo <= yy) & (yy < hi))]
        if todo.size == 0:
            break
    clamped = np.zeros(n, bool)
    clamped[todo] = True
    yc = y[todo]
    yc = np.where(yc < lo, lo, yc)
    yc = np.where(~(yc < hi), np.nextafter(hi, -np.inf), yc)
    y[todo] = yc
    return dict(y=y, comp=comp, z=z, attempts=attempts, clamped=clamped, near=near)


# ---------------------------------------------------------------------------
# the fp32 candidate stream
# ---------------------------------------------------------------------------
def _bm_pair(ta, tb):
    """Box-Muller pair from two upper residuals: radius from ta (clamped to
    >= 2^-24), angle tb in turns; (cos member, sin member)."""
    r = np.sqrt(-2.0 * np.log(np.maximum(ta, 2.0 ** -24)))
    return r * np.cos(2.0 * np.pi * tb), r * np.sin(2.0 * np.pi * tb)


def bound32(b):
    """A bound as the fp32 stream compares against it: the smallest float >= b
    (tpe_sample.hpp bound32), so that low <= y < high holds in fp64 for every
    accepted or clamped fp32 draw.  A bound fp32 holds exactly is unchanged."""
    f = np.float32(b)
    if float(f) < b:
        f = np.nextafter(f, np.float32(np.inf))
    return float(f)


def gmm_draw32(cdf, mu, sigma, key, g, low=None, high=None):
    """Candidates g of the fp32 stream, computed in fp64 from the fp32-rounded
    mu / sigma and the fp32 bounds (bound32).

    Attempt 0 of candidates 4m .. 4m+3 is one call at counter (m, 0, SAMP):
    word j picks candidate 4m+j's component, and the words' residuals inside
    their components' intervals feed Box-Muller -- words 0 / 1 are radius /
    angle of the pair (4m, 4m+1), cos to the first and sin to the second,
    words 2 / 3 those of (4m+2, 4m+3).  A rejected candidate retries with
    calls c = 1..128 at (g, c, RETR): words 0 / 1 pick two components and are
    radius / angle of one pair, two attempts per call, the first accepted
    wins; after call 128 the last attempt is clamped.
    Returns dict(y, comp, z, calls, clamped, near, rejected0, mu32, sigma32):
    calls counts the retry calls used, rejected0 marks a rejected first
    attempt, `near` is the smallest distance of any attempt made to a bound,
    in units of that attempt's sigma_k * max(1, |z|)."""
    cdf = np.asarray(cdf, np.float64)
    mu32 = np.asarray(mu, np.float64).astype(np.float32).astype(np.float64)
    sg32 = np.asarray(sigma, np.float64).astype(np.float32).astype(np.float64)
    g = np.atleast_1d(np.asarray(g, np.int64))
    lo, hi = (bound32(b) for b in _bounds(low, high))
    n = g.size
    r = draw_words(key, g >> 2, 0, SAMP)
    pair = ((g & 2) != 0)
    wa = np.where(pair, r[:, 2], r[:, 0])
    wb = np.where(pair, r[:, 3], r[:, 1])
    ka, ta = component_and_residual(cdf, wa)
    kb, tb = component_and_residual(cdf, wb)
    z0, z1 = _bm_pair(ta, tb)
    second = (g & 1) != 0
    comp = np.where(second, kb, ka)
    z = np.where(second, z1, z0)
    y = mu32[comp] + sg32[comp] * z
    def dist(yy, kk, zz):
        return np.minimum(np.abs(yy - lo), np.abs(yy - hi)) / (
            sg32[kk] * np.maximum(1.0, np.abs(zz)))
    near = dist(y, comp, z)
    calls = np.zeros(n, np.int64)
    todo = np.flatnonzero(~((lo <= y) & (y < hi)))
    rejected0 = np.zeros(n, bool)
    rejected0[todo] = True
    for c in range(1, MAX_RETRY_CALLS + 1):
        if todo.size == 0:
            break
        r = draw_words(key, g[todo], c, RETR)
        k0, t0 = component_and_residual(cdf, r[:, 0])
        k1, t1 = component_and_residual(cdf, r[:, 1])
        c0, s1 = _bm_pair(t0, t1)
        y0 = mu32[k0] + sg32[k0] * c0
        y1 = mu32[k1] + sg32[k1] * s1
        a0 = (lo <= y0) & (y0 < hi)
        a1 = (lo <= y1) & (y1 < hi)
        d0, d1 = dist(y0, k0, c0), dist(y1, k1, s1)
        # the second attempt of a call counts only when the first was rejected
        near[todo] = np.minimum(near[todo], np.where(a0, d0, np.minimum(d0, d1)))
        y[todo] = np.where(a0, y0, y1)
        comp[todo] = np.where(a0, k0, k1)
        z[todo] = np.where(a0, c0, s1)
        calls[todo] = c
        todo = todo[~(a0 | a1)]
    clamped = np.zeros(n, bool)
    clamped[todo] = True
    yc = y[todo]
    yc = np.where(yc < lo, lo, yc)
    yc = np.where(~(yc < hi), float(np.nextafter(np.float32(hi), np.float32(-np.inf))), yc)
    y[todo] = yc
    return dict(y=y, comp=comp, z=z, calls=calls, clamped=clamped, near=near,
                rejected0=rejected0, mu32=mu32, sigma32=sg32)


# ---------------------------------------------------------------------------
# categorical candidates
# ---------------------------------------------------------------------------
def categorical_of_word(cdf, w):
    """Category of the 32-bit words w by the threshold rule on the categories'
    cdf.  The word 2^32 - 1, below no saturated threshold, goes where 2^32 - 2
    goes: to the first category whose threshold saturates (it has mass), never
    to a trailing category of probability zero."""
    return component_thr(thresholds(cdf), np.minimum(_u64(w), np.uint64(0xFFFFFFFE)))


def categorical_draw(cdf, key, g):
    """Category of candidates g: word g & 3 of the call at counter
    (g >> 2, 0, SAMP), by categorical_of_word."""
    g = np.atleast_1d(np.asarray(g, np.int64))
    r = draw_words(key, g >> 2, 0, SAMP)
    w = r[np.arange(g.size), (g & 3)]
    return categorical_of_word(cdf, w)


def categorical_intervals(cdf):
    """(lo, hi): category k takes the words [lo[k], hi[k]) under
    categorical_draw's rule -- thr[k-1] to thr[k], the first category counting
    from 0 and a saturated threshold as 2^32."""
    thr = thresholds(cdf)
    hi = np.where(thr == np.uint64(0xFFFFFFFF), np.uint64(1 << 32), thr)
    return np.concatenate([[np.uint64(0)], hi[:-1]]), hi


# ---------------------------------------------------------------------------
# prior draws
# ---------------------------------------------------------------------------
def _walk(p, u):
    """First k with cumsum(p)[k] > u * sum(p), summed in index order (the
    last category if none)."""
    c = np.cumsum(np.asarray(p, np.float64))  # sequential, as the kernel adds
    t = u * c[-1]
    return np.minimum(np.searchsorted(c[:-1], t, side="right"), c.size - 1) \
        if c.size > 1 else np.zeros(np.shape(u), np.int64)


def prior_draw(rec, p, key, idx):
    """Draws idx of one prior record (fields kind, n_cat, a, b, q, p_off as
    tpe_prior): one call at counter (idx, 0, PRIO); u = u01_f64(x, y), the
    normal kinds take normal_f64(x, y, z).
    Returns dict(v, raw, z): raw is the value before quantization."""
    idx = np.atleast_1d(np.asarray(idx, np.int64))
    r = draw_words(key, idx, 0, PRIO)
    u = u01_f64(r[:, 0], r[:, 1])
    kind, a, b, q = int(rec["kind"]), float(rec["a"]), float(rec["b"]), float(rec["q"])
    z = None
    if kind in (PRIOR_UNIFORM, PRIOR_LOGUNIFORM):
        v = a + (b - a) * u
        if kind == PRIOR_LOGUNIFORM:
            v = np.exp(v)
    elif kind in (PRIOR_NORMAL, PRIOR_LOGNORMAL):
        z = normal_f64(r[:, 0], r[:, 1], r[:, 2])
        v = a + b * z
        if kind == PRIOR_LOGNORMAL:
            v = np.exp(v)
    elif kind == PRIOR_RANDINT:
        v = a + np.minimum(np.floor(u * (b - a)), b - a - 1.0)
    else:
        off, K = int(rec["p_off"]), int(rec["n_cat"])
        v = _walk(np.asarray(p, np.float64)[off:off + K], u).astype(np.float64)
    raw = v
    if q > 0.0:
        v = np.rint(v / q) * q
    return dict(v=v, raw=raw, z=z, u=u)


# ---------------------------------------------------------------------------
# annealing
# ---------------------------------------------------------------------------
def anneal_pick(key, new_id, avg_best_idx, n_active):
    """Rank of a new pick: counter (new_id, 0, ANNL), u1 = 1 - u01_f64(x, y),
    g = ceil(log(u1) / log1p(-1 / avg_best_idx)) - 1 clipped to
    [0, n_active - 1] (0 when 1 / avg_best_idx >= 1).
    Returns (g, quotient): the quotient before the ceil, for callers that
    skip ids whose quotient sits on an integer."""
    new_id = np.atleast_1d(np.asarray(new_id, np.int64))
    r = draw_words(key, new_id, 0, ANNL)
    pg = 1.0 / float(avg_best_idx)
    if not pg < 1.0:
        quo = np.zeros(new_id.size)
        gd = np.zeros(new_id.size)
    else:
        u1 = 1.0 - u01_f64(r[:, 0], r[:, 1])
        quo = np.log(u1) / np.log1p(-pg)
        gd = np.ceil(quo) - 1.0
        gd = np.where(gd >= 0.0, gd, 0.0)
    gd = np.minimum(gd, np.asarray(n_active, np.float64) - 1.0)
    return gd.astype(np.int64), quo


def anneal_variate(key, new_id, kind):
    """The value draw's variate: counter (new_id, 1, ANNL); u01_f64(x, y), or
    normal_f64(x, y, z) for the normal kinds."""
    new_id = np.atleast_1d(np.asarray(new_id, np.int64))
    r = draw_words(key, new_id, 1, ANNL)
    if int(kind) in (PRIOR_NORMAL, PRIOR_LOGNORMAL):
        return normal_f64(r[:, 0], r[:, 1], r[:, 2])
    return u01_f64(r[:, 0], r[:, 1])
