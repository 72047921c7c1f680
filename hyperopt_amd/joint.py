"""A joint (multivariate) Parzen criterion over whole configurations.

``tpe.suggest`` and the pool scores factorise over labels: S(c) = sum_label
(log l - log g).  That model cannot see that a tile size is good only with a
certain unroll factor.  The criterion here scores a configuration under one
mixture over all its always-live labels at once:

    J(c) = log L_below(c) - log L_above(c)

Everything is fp64.

Joint labels.  The labels live in every configuration: ``domain.reachable({})``
in ``domain.params`` order, D of them (D == 0: ValueError).  Labels under a
``switch`` are not joint; ``score_configs(joint=True)`` adds their univariate
terms to J with the pool's fold.

Sets.  The below / above rows of ``collect_history`` + ``split_masks``, the
rows ``tpe.suggest`` conditions on (pending and failed trials sit above).  A
row in which some joint label is not active (foreign trials) is left out of
both sets and does not count.  A set of n rows, in ascending row order, is a
mixture of n + 1 components: trial i with weight ``v_i``, the ramp of
``linear_forgetting`` over n, and the prior last with weight ``prior_weight``;
``log w = log(v / (sum v + prior_weight))``.

Factors.  ``log k_{d,i}(x)`` of joint label d, component i, row value x.  The
prior (mu_p, sigma_p) and the fit coordinate are the univariate fits': midpoint
and width for the uniform kinds, mu and sigma for the normal kinds; log kinds
work on ``t(x) = log(max(x, EPS))``, the others on x.  Component i has
``mu_i = t(obs_i)`` and ``sigma = bandwidth * sigma_p * n ** (-1 / (D + 4))``
(one value per set and label); the prior component has (mu_p, sigma_p).  With
``Phi(v) = 0.5 * (1 + erf((v - mu) / (sqrt(2) sigma)))``:

  continuous   ``-z^2 / 2 - log(sigma sqrt(2 pi)) - log Z``, z = (t(x) - mu) /
               sigma; Z = Phi(hi) - Phi(lo) for the bounded kinds (bounds in
               the fit coordinate), else 1.  The Jacobian of t is left out: it
               is the same in L and G and cancels in J.
  quantized    ``log(Phi(ub) - Phi(lb)) - log Z``; ub / lb are t(x +- q / 2),
               clipped to [lo, hi] where the kind is bounded; for the
               unbounded log kind a lower edge x - q / 2 <= 0 gives Phi = 0
               (a bounded one is clipped to lo first, so the rule never bites
               there).  A mass <= 0 gives -inf.
  categorical, randint   K options with prior probabilities p (1 / K for
               randint): a trial component gives ``log((1[x == c_i] + a p_x) /
               (1 + a))``, a = ``cat_smoothing``; the prior component
               ``log p_x``.  The host builds the K-entry tables (hit, miss,
               prior); the kernel picks by equality.

Mixture.  ``a_i = log w_i + sum_d log k_{d,i}(c_d)``, sequentially over the
joint labels from ``log w_i``; ``log L(c) = m + log sum_i exp(a_i - m)`` with
m = max a_i, summed in component order; m = -inf gives -inf.  NaN
(-inf - -inf) ranks first, as everywhere in the pool code.

``score_numpy`` is this definition in vectorised numpy, for CPU-only users and
for checking; the device path (csrc/tpe_joint.hip, driven by pool.py) builds
the components from the HBM-resident history and scores the pool there.

Drawing (``Pool.sample(joint=True)``, csrc/tpe_joint_sample.hip).
Row g of a joint-drawn pool is one draw from the below set's mixture above:
components 0 .. n - 1 its trials in ascending row order, component n the
prior.  Philox counters are {g lo, g hi, attempt, stream} as everywhere
(oracle/streams.py), the stream word ``STREAM_JOINT`` = 0x4A4F494E ("JOIN"),
distinct from SAMP / RETR / PRIO / ANNL.

  component    key ``component_key(seed)`` = ``_mix64(_mix64(_seed_word(seed)) ^
               STREAM_JOINT)`` (tpe.py's mixing functions; a function of the
               seed alone, no label's hash enters), call (g, 0): word x picks
               the first i with ``cdf[i] > x 2^-32 cdf[-1]``
               (``streams.component_cdf``), ``cdf = sample_cdf(n, lf,
               prior_weight)`` = cumsum of the ramp and the prior's weight.
  label d      key ``tpe.label_key(seed, label_d)``, attempts a = 0, 1, ... at
               (g, a).
    continuous, quantized   ``t = mu + sigma normal_f64(y, z, w)`` with the
               component's (mu, sigma) -- the trial's mu_i and the set's
               bandwidth, or (mu_p, sigma_p).  A bounded kind accepts lo <= t
               < hi; after 256 rejections the last t is clamped to lo or to
               nextafter(hi, -inf) (``draw64``'s rule).  x = exp(t) for the
               log kinds, else t; a quantized label stores rint(x / q) q.
               This is the distribution whose density or mass the factor
               table above states (for a log kind in t: the Jacobian left out
               there belongs to the density in x).
    categorical, randint   attempt 0 only.  A trial component of category c_i
               keeps c_i when ``x 2^-32 (1 + a) < 1``, else takes
               ``categorical_of_word(cumsum(p), y)``; the prior component
               ``categorical_of_word(cumsum(p), x)``.  The stored value is
               the category index (randint(low, high) without ``low``).

A row's values are a function of (seed, g, the set, the label list) alone.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib as _L
from .base import as_domain
from .engine import CATEGORICAL, EPS, _params, categorical_params
from .walk import int_offset

BANDWIDTH = 0.2
CAT_SMOOTHING = 1.0
ROWS_PER_CALL = 1 << 14  # pool rows per tpe_joint_score call: bounds its scratch
STREAM_JOINT = 0x4A4F494E  # "JOIN": the Philox stream word of the joint draws

_erf = np.vectorize(math.erf, otypes=[np.float64])


def joint_labels(domain):
    """The joint labels: live in every configuration, ``domain.params`` order."""
    domain = as_domain(domain)
    live = set(domain.reachable({}))
    return [lab for lab in domain.params if lab in live]


def forgetting_weights(n, lf):
    """The linear-forgetting ramp over n observations, oldest first: ones
    while n < lf, else linspace(1 / n, 1, n - lf) then lf ones."""
    if n == 0:
        return np.zeros(0)
    if n < lf:
        return np.ones(n)
    return np.concatenate([np.linspace(1.0 / n, 1.0, num=n - lf), np.ones(lf)])


def component_key(seed):
    """The 64-bit Philox key of the joint draws' component pick (module doc):
    the suggest seed's word mixed once more, xor the stream word, through the
    splitmix finaliser.  No label enters it."""
    from . import tpe as T
    return T._mix64(T._mix64(T._seed_word(seed)) ^ STREAM_JOINT)


def sample_cdf(n, lf, prior_weight):
    """The running sum of a set's n + 1 component weights, the prior last:
    what the component pick searches."""
    return np.cumsum(np.concatenate([forgetting_weights(n, lf), [float(prior_weight)]]))


def log_weights(n, lf, prior_weight):
    """log w of a set's n + 1 components, the prior last."""
    v = np.concatenate([forgetting_weights(n, lf), [float(prior_weight)]])
    with np.errstate(divide="ignore"):
        return np.log(v / (v[:n].sum() + float(prior_weight)))


class LabelModel(object):
    """A joint label's prior and fit coordinate."""
    __slots__ = ("label", "col", "kind", "is_log", "bounded", "lo", "hi", "q", "mu", "sigma",
                 "n_cat", "p", "offset")


def label_models(domain):
    """One ``LabelModel`` per joint label; ValueError on a label-free space."""
    domain = as_domain(domain)
    labels = list(domain.params)
    out = []
    for lab in joint_labels(domain):
        spec = domain.specs[lab]
        m = LabelModel()
        m.label, m.col = lab, labels.index(lab)
        m.is_log = m.bounded = False
        m.lo = m.hi = m.q = m.mu = m.sigma = 0.0
        m.n_cat, m.p, m.offset = 0, None, 0
        if spec.kind in CATEGORICAL:
            K, _, _, p = categorical_params(spec.kind, spec.args)
            m.kind, m.n_cat = _L.JOINT_CAT, int(K)
            m.p = np.full(K, 1.0 / K) if p is None else np.asarray(p, np.float64)
            m.offset = int(int_offset(spec) or 0)
        else:
            P = _params(spec.kind, spec.args)
            m.kind = _L.JOINT_CONT if P["q"] is None else _L.JOINT_QUANT
            m.is_log, m.bounded = P["family"] == _L.LGMM1, bool(P["bounded"])
            m.lo, m.hi = float(P["low"]), float(P["high"])
            m.q = 0.0 if P["q"] is None else float(P["q"])
            m.mu, m.sigma = float(P["prior_mu"]), float(P["prior_sigma"])
        out.append(m)
    if not out:
        raise ValueError("the joint criterion needs a label that is live in every configuration "
                         "(the space has none)")
    return out


def cat_tables(m, smoothing):
    """(hit, miss, prior) log tables of a discrete label, K entries each."""
    a = float(smoothing)
    with np.errstate(divide="ignore"):
        return (np.log((1.0 + a * m.p) / (1.0 + a)), np.log((a * m.p) / (1.0 + a)), np.log(m.p))


def set_rows(hist, mask, cols):
    """The history rows of a set: those of ``mask`` in which every joint
    column of ``cols`` is active, ascending."""
    mask = np.asarray(mask, bool)
    if hist.tids.size == 0:
        return np.zeros(0, np.int64)
    return np.flatnonzero(mask & np.asarray(hist.active, bool)[:, cols].all(1))


def bandwidths(models, n, bandwidth):
    """sigma of the trial components of a set of n rows, per joint label (0
    for a discrete label, and for n == 0: there is no such component)."""
    D = len(models)
    scale = float(bandwidth) * float(n) ** (-1.0 / (D + 4)) if n else 0.0
    return np.asarray([scale * m.sigma for m in models])


def _fit(m, x):
    with np.errstate(all="ignore"):
        return np.log(np.maximum(x, EPS)) if m.is_log else np.asarray(x, np.float64)


def _cdf(v, mu, sigma):
    with np.errstate(all="ignore"):
        return 0.5 * (1.0 + _erf((v - mu) / (math.sqrt(2.0) * sigma)))


def _log_norm(m, mu, sigma):
    """-log Z per component, Z the mass of [lo, hi] for a bounded kind."""
    if not m.bounded:
        return np.zeros(mu.shape)
    with np.errstate(all="ignore"):
        return -np.log(_cdf(m.hi, mu, sigma) - _cdf(m.lo, mu, sigma))


def _set_log_l(models, hist, rows, x, lf, prior_weight, bandwidth, smoothing):
    """log L of the pool values ``x`` (P, D; stored values) under the set of
    history rows ``rows``."""
    n, P = rows.size, x.shape[0]
    a = np.broadcast_to(log_weights(n, lf, prior_weight), (P, n + 1)).copy()
    sig = bandwidths(models, n, bandwidth)
    for d, m in enumerate(models):
        obs = np.asarray(hist.vals)[rows, m.col] if n else np.zeros(0)
        xd = x[:, d]
        if m.kind == _L.JOINT_CAT:
            hit, miss, prior = cat_tables(m, smoothing)
            c = np.rint(xd).astype(np.int64) - m.offset
            ci = np.rint(obs).astype(np.int64) - m.offset
            term = np.where(c[:, None] == ci[None, :], hit[c][:, None], miss[c][:, None])
            term = np.concatenate([term, prior[c][:, None]], 1)
        else:
            mu = np.concatenate([_fit(m, obs), [m.mu]])
            sigma = np.concatenate([np.full(n, sig[d]), [m.sigma]])
            neg_log_z = _log_norm(m, mu, sigma)
            with np.errstate(all="ignore"):
                if m.kind == _L.JOINT_CONT:
                    z = (_fit(m, xd)[:, None] - mu[None, :]) / sigma[None, :]
                    term = -0.5 * z * z - np.log(sigma * math.sqrt(2.0 * math.pi)) + neg_log_z
                else:
                    lb = xd - 0.5 * m.q
                    tu, tl = _fit(m, xd + 0.5 * m.q), _fit(m, lb)
                    if m.bounded:
                        tu, tl = np.clip(tu, m.lo, m.hi), np.clip(tl, m.lo, m.hi)
                    cu = _cdf(tu[:, None], mu[None, :], sigma[None, :])
                    cl = _cdf(tl[:, None], mu[None, :], sigma[None, :])
                    if m.is_log and not m.bounded:
                        cl = np.where((lb <= 0.0)[:, None], 0.0, cl)
                    mass = cu - cl
                    term = np.where(mass > 0.0, np.log(np.where(mass > 0.0, mass, 1.0)),
                                    -np.inf) + neg_log_z
        with np.errstate(invalid="ignore"):
            a = a + term
    with np.errstate(all="ignore"):
        mx = a.max(1)
        s = np.zeros(P)
        for i in range(n + 1):  # (component order)
            s = s + np.where(a[:, i] == -np.inf, 0.0, np.exp(a[:, i] - mx))
        return np.where(mx == -np.inf, -np.inf, mx + np.log(s))


def score_numpy(domain, hist, vals, active=None, prior_weight=1.0, gamma=0.25,
                linear_forgetting=25, bandwidth=BANDWIDTH, cat_smoothing=CAT_SMOOTHING,
                return_parts=False):
    """J (module doc) of the configurations ``vals`` -- (P, L) stored values in
    ``domain.params`` column order, as ``Pool.vals`` holds them -- under the
    history ``hist`` (``tpe.collect_history``), in numpy: fp64 (P,).  On a
    space without ``switch`` J is the whole criterion; the univariate terms
    of conditional labels are the device path's (``score_configs``).
    ``active`` is accepted for symmetry with ``Pool``: the joint labels are
    live in every row.  ``return_parts``: (J, log L_below, log L_above)."""
    from . import tpe as T
    domain = as_domain(domain)
    models = label_models(domain)
    vals = np.asarray(vals, np.float64)
    cols = [m.col for m in models]
    if active is not None and not np.asarray(active, bool)[:, cols].all():
        raise ValueError("a joint label is not active in some row")
    isb, isa = T.split_masks(hist, gamma) if hist.tids.size else (np.zeros(0, bool),) * 2
    x = vals[:, cols]
    out = [_set_log_l(models, hist, set_rows(hist, mask, cols), x, linear_forgetting,
                      prior_weight, bandwidth, cat_smoothing) for mask in (isb, isa)]
    with np.errstate(invalid="ignore"):
        J = out[0] - out[1]
    return (J, out[0], out[1]) if return_parts else J


# -- device path -----------------------------------------------------------------
class _DeviceJoint(object):
    """A space's joint labels as the kernels take them: the label records on
    the host and on the device, and the discrete labels' tables."""
    __slots__ = ("models", "host", "dev", "tables", "n_tables")


def _device_labels(eng, models, smoothing):
    t = eng.torch
    rec = np.zeros(len(models), _L.JOINT_LABEL_DTYPE)
    tabs, off = [], 0
    for d, m in enumerate(models):
        r = rec[d]
        r["kind"], r["col"], r["n_cat"] = m.kind, m.col, m.n_cat
        r["flags"] = (_L.JOINT_LOG if m.is_log else 0) | (_L.JOINT_BOUNDED if m.bounded else 0)
        r["lo"], r["hi"], r["q"] = m.lo, m.hi, m.q
        r["prior_mu"], r["prior_sigma"] = m.mu, m.sigma
        r["shift"] = m.offset
        if m.kind == _L.JOINT_CAT:
            r["tab_off"] = off
            tabs.extend(cat_tables(m, smoothing))
            off += 3 * m.n_cat
        else:
            with np.errstate(divide="ignore"):
                r["prior_r"] = 1.0 / (math.sqrt(2.0) * m.sigma)
    dj = _DeviceJoint()
    dj.models, dj.host = models, rec
    dj.dev = t.from_numpy(rec.view(np.uint8).copy()).to(eng.device)
    dj.n_tables = off
    dj.tables = t.from_numpy(np.concatenate(tabs)).to(eng.device) if tabs else None
    return dj


def _prepare_set(eng, dj, seen, hist_cols, rows, lf, prior_weight, bandwidth, sp):
    """One set on the device: (set tensor, n).  ``seen``: pool._seen_rows'
    view of the history; ``rows``: the set's rows as positions of that view."""
    t, lib = eng.torch, eng.lib
    _alive, sv, sa, sld, _srows, _n = seen
    D, n = len(dj.models), int(rows.size)
    sig = bandwidths(dj.models, n, bandwidth)
    # (a discrete label, and every label of an empty set, has no bandwidth:
    # 0 goes up for its 1 / (sqrt(2) sigma), never an infinity)
    some = sig > 0.0
    r = np.where(some, 1.0 / (math.sqrt(2.0) * np.where(some, sig, 1.0)), 0.0)
    head = np.concatenate([log_weights(n, lf, prior_weight), sig, r])
    dset = t.empty(lib.tpe_joint_set_doubles(D, n), dtype=t.float64, device=eng.device)
    dset[:head.size].copy_(t.from_numpy(head))
    drows = t.from_numpy(np.ascontiguousarray(rows, np.int32)).to(eng.device) if n else None
    _L.check(lib.tpe_joint_prep(dj.host.ctypes.data, dj.dev.data_ptr(), D, sv, sa, sld, hist_cols,
                                None if drows is None else drows.data_ptr(), n,
                                dset.data_ptr(), sp), "tpe_joint_prep")
    return dset, n, drows


def prepare_sets(eng, domain, hist, seen, isb, isa, n_cols, prior_weight, linear_forgetting,
                 bandwidth, cat_smoothing):
    """The space's label records and both sets on the device: (dj, [below,
    above], stream pointer), a set as ``_prepare_set`` returns it.  ``seen``:
    ``pool._seen_rows(eng, hist)``; ``n_cols``: the columns of the history
    (and of the pool: both are in ``domain.params`` order)."""
    t = eng.torch
    models = label_models(domain)
    dj = _device_labels(eng, models, cat_smoothing)
    sp = ctypes.c_void_p(t.cuda.current_stream(eng.device).cuda_stream)
    cols = [m.col for m in models]
    view = hist.rows if (seen[4] is not None) else None  # (positions -> rows of the mirror)
    sets = []
    for mask in (isb, isa):
        rows = set_rows(hist, mask, cols)
        if view is not None:
            rows = np.asarray(view)[rows]
        sets.append(_prepare_set(eng, dj, seen, n_cols, rows, linear_forgetting, prior_weight,
                                 bandwidth, sp))
    return dj, sets, sp


def score_device(eng, domain, hist, seen, isb, isa, d_vals, ld, n_cols, P, out, prior_weight,
                 linear_forgetting, bandwidth, cat_smoothing, parts=None, prepared=None):
    """J of rows [0, P) of the label-major device pool ``d_vals`` (leading
    dimension ``ld``, ``n_cols`` columns) into the device vector ``out``.
    ``seen``: ``pool._seen_rows(eng, hist)``; ``parts``: a device tensor whose
    rows 0 and 1 (>= P long) receive log L_below and log L_above;
    ``prepared``: ``prepare_sets``' result for the same arguments, where the
    caller has made it already."""
    t, lib = eng.torch, eng.lib
    if prepared is None:
        prepared = prepare_sets(eng, domain, hist, seen, isb, isa, n_cols, prior_weight,
                                linear_forgetting, bandwidth, cat_smoothing)
    dj, sets, sp = prepared
    D = len(dj.models)
    tab = None if dj.tables is None else dj.tables.data_ptr()
    win = min(max(P, 1), ROWS_PER_CALL)
    need = max(lib.tpe_joint_scratch_bytes(win, n) for _, n, _ in sets)
    scratch = t.empty(max(need, 16), dtype=t.uint8, device=eng.device)
    above = t.empty(win, dtype=t.float64, device=eng.device) if parts is None else None

    def score(which, r0, k, sub, dst):
        dset, n, _ = sets[which]
        _L.check(lib.tpe_joint_score(dj.host.ctypes.data, dj.dev.data_ptr(), D, tab, dj.n_tables,
                                     dset.data_ptr(), n, d_vals.data_ptr(), ld, n_cols, r0, k,
                                     sub, dst, scratch.data_ptr(), sp), "tpe_joint_score")

    for r0 in range(0, P, win):
        k = min(win, P - r0)
        # above first: the below call subtracts it (with ``parts`` it lands in
        # row 1 and is the subtrahend from there)
        la = above.data_ptr() if parts is None else parts[1].data_ptr() + 8 * r0
        score(1, r0, k, None, la)
        if parts is not None:
            # log L_below by itself costs one more call: J keeps the bits of the
            # call without ``parts`` because it is made by the same call
            score(0, r0, k, None, parts[0].data_ptr() + 8 * r0)
        score(0, r0, k, la, out.data_ptr() + 8 * r0)


def sample_device(eng, prepared, seed, prior_weight, linear_forgetting, cat_smoothing, d_vals, ld,
                  n_cols, row_base, n_rows, comp_out=None):
    """Rows [row_base, row_base + n_rows) of the joint draw (module doc) from
    the below set of ``prepared`` (``prepare_sets``) into rows [0, n_rows) of
    the joint labels' columns of the label-major device block ``d_vals``
    (tpe_joint_sample).  ``comp_out``: a device int32 tensor for the rows'
    components.  Three small uploads: the component cdf, the discrete labels'
    cdf table and the keys."""
    from . import tpe as T
    t, lib = eng.torch, eng.lib
    dj, sets, sp = prepared
    dset, n, _ = sets[0]
    cdf = t.from_numpy(sample_cdf(n, linear_forgetting, prior_weight)).to(eng.device)
    cats = [np.cumsum(m.p) for m in dj.models if m.kind == _L.JOINT_CAT]
    cat_cdf = t.from_numpy(np.concatenate(cats)).to(eng.device) if cats else None
    keys = np.asarray([T.label_key(seed, m.label) for m in dj.models] + [component_key(seed)],
                      np.uint64)
    d_keys = t.from_numpy(keys.view(np.int64)).to(eng.device)
    _L.check(lib.tpe_joint_sample(dj.host.ctypes.data, dj.dev.data_ptr(), len(dj.models),
                                  dset.data_ptr(), n, cdf.data_ptr(),
                                  None if cat_cdf is None else cat_cdf.data_ptr(),
                                  0 if cat_cdf is None else cat_cdf.numel(), d_keys.data_ptr(),
                                  1.0 + float(cat_smoothing), row_base, n_rows,
                                  d_vals.data_ptr(), ld, n_cols,
                                  None if comp_out is None else comp_out.data_ptr(), sp),
             "tpe_joint_sample")
