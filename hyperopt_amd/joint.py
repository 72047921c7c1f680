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

Groups (``joint="tree"``, csrc/tpe_joint_tree.hip).  The
criterion above covers the labels live in every configuration; on a space
that opens with a ``switch`` that is the selector alone.  ``joint="tree"``
gives every label a joint mixture: one per group of labels that share an
activation condition.

  groups       ``domain.live_program()`` gives every label a tuple of clauses.
               Labels with identical clause tuples form a group, its labels in
               ``domain.params`` order; groups are ordered by the position of
               their first label (``joint_groups``).  The group with the empty
               clause is the root group: its labels are ``joint_labels(domain)``
               and it comes first.  A space without a program (a ``switch`` on
               an expression) that is not flat raises ValueError; a label-free
               space raises as above.  Per group D_g <= ``TPE_COND_MAX_LABELS``
               and K <= ``TPE_JOINT_MAX_CAT``.
  sets         the below / above split is the global one (``split_masks``).
               Group g's below (above) set is the rows of that side in which
               every label of g is active -- ``set_rows`` with the group's
               columns; a row with only some of them (foreign trials) is left
               out and does not count in n.  Weights, the prior component,
               factors, ``cat_smoothing`` and the mixture sum are the ones
               above with D_g for D in the bandwidth exponent and n the
               group's set size.  An empty set (a branch never tried) is the
               prior alone.
  criterion    ``J_g(c) = log L_below,g(c) - log L_above,g(c)`` over group g's
               labels, for the rows c in which g is live.  S(c) is the
               sequential fp64 sum, in group order, of J_g(c) over the groups
               live in row c, starting as S = J_root (assigned, not added to
               0.0): on a flat space S has the bits of ``joint=True``.  Every
               label is joint: no univariate term is added.  NaN ranks first.
               ``score_configs(joint="tree", return_terms=True)`` gives (S,
               terms, J): ``terms`` all NaN, J the (P, G) matrix of J_g, NaN
               where group g is not live in the row; S is exactly the
               sequential fold of J's live columns.
  drawing      every group's labels are drawn for all P rows from that group's
               below mixture by the rule above (entries of rows in which the
               group turns out not to be live are ignored, as a sampled pool
               ignores them for any label under a ``switch``).  Label keys
               stay ``tpe.label_key(seed, label)``.  The root group's
               component key stays ``component_key(seed)``; group g's is
               ``group_component_key(seed, first label of g)`` =
               ``_mix64(label_key(seed, first label) ^ STREAM_JOINT)``, so no
               two groups pick their components from one Philox word.  One
               ``tpe_rows_active`` after all groups gives the activity, and
               the pool is born with the tree S of its own rows.

Grid pools (``GridPool(..., joint=True)``, csrc/tpe_grid_joint.hip, DESIGN
3.5.7).  J is not separable over a grid's axes, but inside a component the
factor of label d depends on the label's value alone, and on a grid that is one
of the axis's values: per set the factors form a table of (sum of the axis
lengths) x (n + 1) doubles, built once by the factor expressions above, and a
row's ``a_i`` is ``log w_i`` plus one table entry per label, added in the same
order -- the bits of the materialised pool (``score_grid_device``).

Batches (``batch="liar"``, csrc/tpe_joint_lie.hip).  The k rows
of one call are the k best under one score vector: picked as if each were the
only one.  Across calls a pending trial sits in the above set and pushes the
score down around itself; inside a call ``batch="liar"`` does the same: the
rows are picked one at a time on the device, and each pick joins the above
mixture as the pending trial it is about to become.  L_above is a sum of
product kernels, so that is one more component: O(P D) per pick.

  inputs       per pool row r: ``S_0[r]``, the score under ``joint=True`` (J
               plus the folded terms of the labels under a ``switch``), bits
               unchanged; ``A_0[r] = log L_above(r)``.  The above set as
               prepared: n rows, sigma = ``bandwidths(models, n, bandwidth)``
               (n == 0: ``bandwidths(models, 1, bandwidth)``) and
               ``W = sum(forgetting_weights(n, lf)) + prior_weight``, the
               denominator of ``log_weights``.
  lie          pick p is a trial component of the above set whose observation
               is row p's stored values: ``c_p(r) = log(lie_weight) + sum_d
               log k_d(r_d)``, sequentially over the joint labels from
               ``log(lie_weight)``, ``log k_d`` the "Factors" entry of a trial
               component with ``mu = t(x_{p,d})`` (the category of p for a
               discrete label) and the set's sigma_d: the same -log Z,
               quantized mass, clipping and hit / miss tables -- what
               ``tpe_joint_prep`` would write for a history row that held p.
  update       ``U_0[r] = log W + A_0[r]``; after pick j ``U_j[r] = m +
               log(exp(U_{j-1}[r] - m) + exp(c_{p_j}(r) - m))``, m the larger
               of the two, U's term first; m = -inf gives -inf, and c = -inf
               leaves U's bits.
  score        ``S_j[r] = S_0[r] - (U_j[r] - U_0[r])`` where ``U_0[r]`` is
               finite, else ``S_0[r]``.  The penalty is >= 0 and unnormalised
               on purpose: the factor W / (W + j) is the same for every row.
  picks        p_1 is the first untaken row of S_0 in ``tpe_pool_topk``'s order
               (larger first, NaN before everything, equal scores to the
               smaller row); p_{j+1} the first row of S_j among the rows that
               are untaken, not yet picked, and pass ``distinct``'s mask where
               one is given.  The run stops when no row is left.  k = 1 is the
               plain result, bit for bit.

On a conditional space the lie acts through the always-live labels only: two
rows that differ under a ``switch`` alone get the same penalty.
``liar_numpy`` is this definition in numpy; ``liar_device`` enqueues all k
picks in one call (a pick's row is read on the device) and reads back the rows.

Chains (``joint="chain"``, csrc/tpe_joint_chain.hip).  The
groups above are independent mixtures: a label at the root (a tile size) that
is good only together with a label inside one branch (that variant's unroll
factor) is ranked by two separate terms.  ``joint="chain"`` conditions every
group on the labels around it by the chain rule: group g contributes the ratio
L(ctx + g) / L(ctx).

  groups       those of ``joint_groups(domain)``: the same groups, the same
               order, the same global split.
  context      ``ctx(g)`` of a group g that is not the root: the labels l
               outside g, in ``domain.params`` order, with both properties
               (``prog`` = ``domain.live_program()``): (1) l is live whenever g
               is -- for every clause c of g some clause of ``prog[l]`` is a
               subset of c; (2) l is not a selector that every clause of g
               names with one and the same branch index (such a selector is
               constant on g's rows).  So ctx of a group under one branch of a
               root switch is the root group without that switch's selector;
               ctx of a nested group also holds its ancestor groups' labels
               without the fixed selectors; ctx of a group reachable from two
               branches keeps the selector, because it varies.  ``ctx(root)``
               is empty (``joint_contexts``).
  sets         group g's below (above) set is the rows of that side in which
               every label of ``ctx(g) + g`` is active (``set_rows`` with those
               columns).  The mixture's label list is ``ctx(g)`` first, then
               g's labels, each in ``domain.params`` order: D = D_ctx + D_g.
               Weights, the prior component, -log Z, quantized masses, hit /
               miss tables and ``cat_smoothing`` are those of "Factors" /
               "Mixture"; ``sigma = bandwidth * sigma_p * n ** (-1 / (D + 4))``
               with this D and this n.  D <= ``TPE_COND_MAX_LABELS`` and K <=
               ``TPE_JOINT_MAX_CAT``, else ValueError.
  term         for one set ``a_i^ctx = log w_i + sum over the D_ctx context
               labels`` (sequential), and ``a_i`` continues the same sum over
               g's labels.  ``log L_ctx`` and ``log L`` are the two
               log-sum-exps by the "Mixture" rule.  The marginal is the same
               mixture with g's factors dropped -- the same components, weights
               and sigmas -- not a refit with D_ctx.  ``C_g(c) = (log L_below -
               log L_ctx,below) - (log L_above - log L_ctx,above)``, in that
               order of operations.  NaN from -inf - -inf propagates and ranks
               first.
  criterion    S = J_root, assigned (``score_device`` on the root group); then
               S = S + C_g in group order over the groups live in the row.  A
               group with an empty context has C_g = J_g and is scored exactly
               as under ``"tree"``: a flat space has the bits of
               ``joint=True``, a space whose groups all have empty contexts the
               bits of ``joint="tree"``.  ``score_configs(joint="chain",
               return_terms=True)`` gives (S, terms, C): ``terms`` all NaN, C
               the (P, G) matrix with J_root in column 0 and C_g in column g,
               NaN where g is not live; S is exactly the fold of C's live
               columns.
  drawing      ``Pool.sample(joint="chain")`` draws its rows exactly as
               ``joint="tree"`` does, from the tree fits (the columns are bit
               for bit the same for one seed): the draw is a proposal, the
               ranking is this criterion, and the pool is born with the chain S
               of its rows.

Not built: a draw conditioned on the row's context (component weights ``w_i *
prod_ctx k``: ``joint="chain"`` draws as ``"tree"`` does).  ``joint="chain"``
on a ``GridPool`` (the factor tables hold one group's axes; a chain term needs
the context's as well).  ``batch="liar"`` under ``joint="tree"`` and
``joint="chain"`` (it needs log L_above per group, which ``score_tree_device``
does not keep), on a ``GridPool`` (a grid has no row values to lie with) and
under the factorised criterion (its adaptive bandwidths depend on the sorted
neighbours: no component can be added without a refit).
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
# a grid pool (``score_grid_device``): block rows per tpe_grid_joint_score call,
# which bounds its scratch, and the bytes of one factor table (a starting
# value, not a measured one)
GRID_ROWS_PER_CALL = 1 << 14
GRID_JOINT_TABLE_BYTES = 256 << 20

_erf = np.vectorize(math.erf, otypes=[np.float64])


def joint_labels(domain):
    """The joint labels: live in every configuration, ``domain.params`` order."""
    domain = as_domain(domain)
    live = set(domain.reachable({}))
    return [lab for lab in domain.params if lab in live]


class Group(object):
    """A group of labels that share an activation condition: ``clauses`` (the
    labels' common entry of ``domain.live_program()``; ``()`` for the root
    group) and ``labels`` in ``domain.params`` order."""
    __slots__ = ("clauses", "labels")

    def __init__(self, clauses, labels):
        self.clauses, self.labels = clauses, labels

    def __repr__(self):
        return "Group(%r, %r)" % (self.clauses, self.labels)


def joint_groups(domain):
    """The groups of ``joint="tree"`` (module doc, "Groups"), the root group
    first: a list of ``Group``.  ValueError on a label-free space, and on a
    space without a liveness program that is not flat."""
    domain = as_domain(domain)
    root = joint_labels(domain)
    if not root:
        label_models(domain)  # (raises: the space has no joint label)
    prog = domain.live_program()
    if prog is None:
        if len(root) == len(domain.params):
            return [Group(((),), root)]
        raise ValueError("joint='tree' needs the space's liveness as a program, and this space "
                         "has none: a switch is selected by something other than a bare "
                         "hp.choice / hp.pchoice / hp.randint(n) label")
    groups = {}
    for lab in domain.params:  # (a dict keeps the order of first insertion)
        groups.setdefault(prog[lab], []).append(lab)
    out = [Group(clauses, labs) for clauses, labs in groups.items()]
    # the walk that orders ``domain.params`` meets a switch's selector before
    # its branches, so the first label is always live: the root group leads
    assert out[0].clauses == ((),) and out[0].labels == root
    return out


def joint_contexts(domain):
    """``ctx(g)`` of ``joint="chain"`` (module doc, "Chains"): one label list
    per group of ``joint_groups(domain)``, in ``domain.params`` order; empty
    for the root group."""
    domain = as_domain(domain)
    groups = joint_groups(domain)
    prog = domain.live_program()
    out = [[]]
    for grp in groups[1:]:
        clauses = [dict(c) for c in grp.clauses]
        ctx = []
        for lab in domain.params:
            if lab in grp.labels:
                continue
            # (1) live whenever the group is
            if not all(any(set(lc) <= set(c.items()) for lc in prog[lab]) for c in clauses):
                continue
            # (2) not a selector held at one branch on all the group's rows
            if all(lab in c for c in clauses) and len(set(c[lab] for c in clauses)) == 1:
                continue
            ctx.append(lab)
        out.append(ctx)
    return out


def group_component_key(seed, first_label):
    """The Philox key of the component pick of the group whose first label is
    ``first_label`` (not the root group: that one keeps ``component_key``)."""
    from . import tpe as T
    return T._mix64(T.label_key(seed, first_label) ^ STREAM_JOINT)


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


def label_models(domain, group=None):
    """One ``LabelModel`` per joint label -- per label of the list ``group``
    where one is given (a group of ``joint_groups``); ValueError on a
    label-free space."""
    domain = as_domain(domain)
    labels = list(domain.params)
    out = []
    for lab in (joint_labels(domain) if group is None else group):
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


def split_sets(hist, gamma):
    """The below / above row masks of ``hist`` (``tpe.split_masks``); two empty
    masks for an empty history."""
    from . import tpe as T
    return T.split_masks(hist, gamma) if hist.tids.size else (np.zeros(0, bool),) * 2


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


def _density_terms(m, xd, mu, sigma):
    """log k of the stored values ``xd`` (P,) of a continuous or quantized
    label under components (mu, sigma) (C,): (P, C)."""
    neg_log_z = _log_norm(m, mu, sigma)
    with np.errstate(all="ignore"):
        if m.kind == _L.JOINT_CONT:
            z = (_fit(m, xd)[:, None] - mu[None, :]) / sigma[None, :]
            return -0.5 * z * z - np.log(sigma * math.sqrt(2.0 * math.pi)) + neg_log_z
        lb = xd - 0.5 * m.q
        tu, tl = _fit(m, xd + 0.5 * m.q), _fit(m, lb)
        if m.bounded:
            tu, tl = np.clip(tu, m.lo, m.hi), np.clip(tl, m.lo, m.hi)
        cu = _cdf(tu[:, None], mu[None, :], sigma[None, :])
        cl = _cdf(tl[:, None], mu[None, :], sigma[None, :])
        if m.is_log and not m.bounded:
            cl = np.where((lb <= 0.0)[:, None], 0.0, cl)
        mass = cu - cl
        return np.where(mass > 0.0, np.log(np.where(mass > 0.0, mass, 1.0)),
                        -np.inf) + neg_log_z


def _log_sum_exp(a):
    """The "Mixture" rule over the (P, C) matrix of a_i, in component order."""
    with np.errstate(all="ignore"):
        mx = a.max(1)
        s = np.zeros(a.shape[0])
        for i in range(a.shape[1]):  # (component order)
            s = s + np.where(a[:, i] == -np.inf, 0.0, np.exp(a[:, i] - mx))
        return np.where(mx == -np.inf, -np.inf, mx + np.log(s))


def _set_log_l(models, hist, rows, x, lf, prior_weight, bandwidth, smoothing, n_ctx=0):
    """log L of the pool values ``x`` (P, D; stored values) under the set of
    history rows ``rows``.  ``n_ctx`` > 0: (log L, log L_ctx), the second the
    same mixture cut off after its first ``n_ctx`` labels ("Chains")."""
    n, P = rows.size, x.shape[0]
    a = np.broadcast_to(log_weights(n, lf, prior_weight), (P, n + 1)).copy()
    sig = bandwidths(models, n, bandwidth)
    ctx = None
    for d, m in enumerate(models):
        if n_ctx and d == n_ctx:
            ctx = _log_sum_exp(a)
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
            term = _density_terms(m, xd, mu, sigma)
        with np.errstate(invalid="ignore"):
            a = a + term
    return (_log_sum_exp(a), ctx) if n_ctx else _log_sum_exp(a)


def score_numpy(domain, hist, vals, active=None, prior_weight=1.0, gamma=0.25,
                linear_forgetting=25, bandwidth=BANDWIDTH, cat_smoothing=CAT_SMOOTHING,
                return_parts=False, tree=False):
    """J (module doc) of the configurations ``vals`` -- (P, L) stored values in
    ``domain.params`` column order, as ``Pool.vals`` holds them -- under the
    history ``hist`` (``tpe.collect_history``), in numpy: fp64 (P,).  On a
    space without ``switch`` J is the whole criterion; the univariate terms
    of conditional labels are the device path's (``score_configs``).
    ``active`` is accepted for symmetry with ``Pool``: the joint labels are
    live in every row.  ``return_parts``: (J, log L_below, log L_above).

    ``tree=True``: S of ``joint="tree"`` (module doc, "Groups") -- the whole
    criterion on any space with a liveness program.  ``active`` ((P, L); None:
    where ``vals`` is not NaN) says where a group is live.  ``return_parts``:
    (S, J, log L_below, log L_above), the last three (P, G) matrices, NaN
    where the group is not live.

    ``tree="chain"``: S of ``joint="chain"`` (module doc, "Chains").
    ``return_parts``: (S, C, log L_below, log L_above, log L_ctx,below, log
    L_ctx,above), the last five (P, G) matrices, NaN where the group is not
    live; the two marginals also NaN in the columns of the groups with an empty
    context (the root's among them), whose C_g is J_g."""
    domain = as_domain(domain)
    if tree:
        return _score_numpy_tree(domain, hist, vals, active, prior_weight, gamma,
                                 linear_forgetting, bandwidth, cat_smoothing, return_parts,
                                 tree == "chain")
    models = label_models(domain)
    vals = np.asarray(vals, np.float64)
    cols = [m.col for m in models]
    if active is not None and not np.asarray(active, bool)[:, cols].all():
        raise ValueError("a joint label is not active in some row")
    isb, isa = split_sets(hist, gamma)
    x = vals[:, cols]
    out = [_set_log_l(models, hist, set_rows(hist, mask, cols), x, linear_forgetting,
                      prior_weight, bandwidth, cat_smoothing) for mask in (isb, isa)]
    with np.errstate(invalid="ignore"):
        J = out[0] - out[1]
    return (J, out[0], out[1]) if return_parts else J


def _score_numpy_tree(domain, hist, vals, active, prior_weight, gamma, lf, bandwidth, smoothing,
                      return_parts, chain=False):
    groups = joint_groups(domain)
    contexts = joint_contexts(domain) if chain else [[]] * len(groups)
    vals = np.asarray(vals, np.float64)
    active = ~np.isnan(vals) if active is None else np.asarray(active, bool)
    P, G = vals.shape[0], len(groups)
    isb, isa = split_sets(hist, gamma)
    # J (with ``chain``: C), log L_below, log L_above, and the context marginals
    parts = np.full((5, P, G), np.nan)
    S = None
    for g, (grp, ctx) in enumerate(zip(groups, contexts)):
        own = [m.col for m in label_models(domain, grp.labels)]
        live = active[:, own].all(1)
        if (active[:, own].any(1) != live).any() or (g == 0 and not live.all()):
            raise ValueError("a group's labels are not active together in some row")
        models = label_models(domain, ctx + grp.labels)
        cols = [m.col for m in models]
        if not active[live][:, cols].all():
            raise ValueError("a context label is not active in a row in which its group is live")
        x = vals[live][:, cols]
        out = [_set_log_l(models, hist, set_rows(hist, mask, cols), x, lf, prior_weight,
                          bandwidth, smoothing, len(ctx)) for mask in (isb, isa)]
        with np.errstate(invalid="ignore"):
            if ctx:
                (lb, cb), (la, ca) = out
                parts[3, live, g], parts[4, live, g] = cb, ca
                parts[0, live, g] = (lb - cb) - (la - ca)
            else:
                lb, la = out
                parts[0, live, g] = lb - la
            parts[1, live, g], parts[2, live, g] = lb, la
            # (S starts as J_root, assigned: the root group is live in every row)
            S = parts[0, :, 0].copy() if g == 0 else np.where(live, S + parts[0, :, g], S)
    if not return_parts:
        return S
    return (S,) + tuple(parts) if chain else (S, parts[0], parts[1], parts[2])


# -- batches (module doc, "Batches") ---------------------------------------------
def lie_sigma(models, n, bandwidth):
    """The bandwidths a lie takes: the above set's, or a set of one row's
    where the above set is empty."""
    return bandwidths(models, n if n else 1, bandwidth)


def lie_log_total(n, lf, prior_weight):
    """log W: W the denominator of ``log_weights(n, lf, prior_weight)``."""
    return math.log(forgetting_weights(n, lf).sum() + float(prior_weight))


def _lie_component(models, x, p, sig, smoothing, log_lie):
    """c_p(r) for every row r of ``x`` (P, D; stored values)."""
    c = np.full(x.shape[0], log_lie)
    for d, m in enumerate(models):
        xd = x[:, d]
        if m.kind == _L.JOINT_CAT:
            hit, miss, _prior = cat_tables(m, smoothing)
            q = np.rint(xd).astype(np.int64) - m.offset
            term = np.where(q == q[p], hit[q], miss[q])
        else:
            term = _density_terms(m, xd, np.asarray([_fit(m, xd[p])]), np.asarray([sig[d]]))[:, 0]
        with np.errstate(invalid="ignore"):
            c = c + term
    return c


def _first_row(S, gone):
    """The first row of S outside ``gone`` in ``tpe_pool_topk``'s order, or -1."""
    free = np.flatnonzero(~gone)
    if not free.size:
        return -1
    s = S[free]
    nan = np.isnan(s)
    return int(free[np.argmax(nan)] if nan.any() else free[np.argmax(s)])


def liar_numpy(domain, hist, vals, k, taken=None, distinct=None, lie_weight=1.0, S0=None, A0=None,
               prior_weight=1.0, gamma=0.25, linear_forgetting=25, bandwidth=BANDWIDTH,
               cat_smoothing=CAT_SMOOTHING):
    """The batch of module doc "Batches" in numpy: (rows, S_at_pick, S_k) --
    the picks in order (int64, at most k), the score each was picked at, and
    the score of every row after the last pick.  ``vals``: (P, L) stored values
    as ``Pool.vals`` holds them; ``taken`` / ``distinct``: row masks (nonzero:
    not to be picked).  ``S0`` / ``A0``: the score and log L_above to start
    from where the caller has them (a device's, or S with the folded terms of
    a conditional space); else ``score_numpy``'s J and log L_above."""
    domain = as_domain(domain)
    if not lie_weight > 0.0 or not np.isfinite(lie_weight):
        raise ValueError("lie_weight=%r must be > 0 and finite" % (lie_weight,))
    models = label_models(domain)
    vals = np.asarray(vals, np.float64)
    P = vals.shape[0]
    cols = [m.col for m in models]
    if S0 is None or A0 is None:
        J, _below, above = score_numpy(domain, hist, vals, None, prior_weight, gamma,
                                       linear_forgetting, bandwidth, cat_smoothing,
                                       return_parts=True)
        S0 = J if S0 is None else S0
        A0 = above if A0 is None else A0
    S0, A0 = np.asarray(S0, np.float64), np.asarray(A0, np.float64)
    n = int(set_rows(hist, split_sets(hist, gamma)[1], cols).size)
    sig = lie_sigma(models, n, bandwidth)
    x = vals[:, cols]
    gone = np.zeros(P, bool)
    for mask in (taken, distinct):
        if mask is not None:
            gone |= np.asarray(mask)[:P] != 0
    U0 = lie_log_total(n, linear_forgetting, prior_weight) + A0
    U, S = U0.copy(), S0.copy()
    rows, at = [], []
    for _ in range(min(max(int(k), 0), P)):
        p = _first_row(S, gone)
        if p < 0:
            break
        rows.append(p)
        at.append(S[p])
        gone[p] = True
        c = _lie_component(models, x, p, sig, cat_smoothing, math.log(lie_weight))
        with np.errstate(all="ignore"):
            m = np.where(c > U, c, U)
            both = m + np.log(np.exp(U - m) + np.exp(c - m))
            U = np.where(c == -np.inf, U, np.where(m == -np.inf, -np.inf, both))
            S = np.where(np.isfinite(U0), S0 - (U - U0), S0)
    return np.asarray(rows, np.int64), np.asarray(at, np.float64), S


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


def stream_ptr(eng):
    """The current stream of ``eng``'s device as the C entries take it."""
    return ctypes.c_void_p(eng.torch.cuda.current_stream(eng.device).cuda_stream)


def _prepare_set(eng, dj, seen, hist_cols, rows, lf, prior_weight, bandwidth, sp):
    """One set on the device: (set tensor, n, row list).  ``seen``: the history
    on the device (``fit``); ``rows``: the set's rows as rows of that mirror."""
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


class JointFit(object):
    """One mixture pair fitted to a history, on the device (``fit``): the
    engine, the label records ``dj``, ``sets`` = [below, above] as
    ``_prepare_set`` returns them, the stream pointer ``sp``, ``group`` (the
    labels of its group of ``joint_groups``; None: the joint labels), ``n_ctx``
    (with ``tree="chain"`` the number of context labels that lead ``dj``'s
    list, before the group's own; else 0) and the settings it was made with."""
    __slots__ = ("eng", "dj", "sets", "sp", "group", "n_ctx", "prior_weight",
                 "linear_forgetting", "bandwidth", "cat_smoothing")


def fit(eng, domain, hist, seen, gamma, n_cols, prior_weight, linear_forgetting, bandwidth,
        cat_smoothing, tree=False):
    """The joint model of the history ``hist`` under the split of ``gamma``:
    [JointFit] -- the joint labels' alone, or with ``tree`` one per group of
    ``joint_groups(domain)``, the root group first.  Per fit the label records
    go up, then both sets are built there (tpe_joint_prep).  ``tree="chain"``:
    a group with a context is fitted over ``ctx + g`` (module doc, "Chains")
    and records ``n_ctx``; the root's fit, and that of any group with an empty
    context, is the one ``tree=True`` makes.

    ``seen``: the history on the device, the tuple (keep-alive tensors, values
    pointer, activity pointer, leading dimension, rows pointer or None, T) --
    label-major fp64 values and activity bytes in ``domain.params`` column
    order, and T the number of history rows; where the two are a longer
    mirror of which ``hist`` is a view, the int32 device list of its rows
    (``hist.rows``), else None: position t is history row t.  ``n_cols``: the
    columns of the history (and of the pool: the same order)."""
    isb, isa = split_sets(hist, gamma)
    view = hist.rows if (seen[4] is not None) else None  # (positions -> rows of the mirror)
    fits = []
    groups = [grp.labels for grp in joint_groups(domain)] if tree else [None]
    contexts = joint_contexts(domain) if tree == "chain" else [[]] * len(groups)
    for group, ctx in zip(groups, contexts):
        f = JointFit()
        f.eng, f.group, f.n_ctx = eng, group, len(ctx)
        f.prior_weight, f.linear_forgetting = prior_weight, linear_forgetting
        f.bandwidth, f.cat_smoothing = bandwidth, cat_smoothing
        models = label_models(domain, ctx + group if ctx else group)
        if ctx and (len(models) > _L.COND_MAX_LABELS or
                    max(m.n_cat for m in models) > _L.JOINT_MAX_CAT):
            raise ValueError("joint='chain': the group of %r with its context has %d labels (at "
                             "most %d) / a label of %d options (at most %d)"
                             % (group[0], len(models), _L.COND_MAX_LABELS,
                                max(m.n_cat for m in models), _L.JOINT_MAX_CAT))
        f.dj = _device_labels(eng, models, cat_smoothing)
        f.sp = stream_ptr(eng)
        cols = [m.col for m in models]
        f.sets = []
        for mask in (isb, isa):
            rows = set_rows(hist, mask, cols)
            if view is not None:
                rows = np.asarray(view)[rows]
            f.sets.append(_prepare_set(eng, f.dj, seen, n_cols, rows, linear_forgetting,
                                       prior_weight, bandwidth, f.sp))
        fits.append(f)
    return fits


def score_device(fit, d_vals, ld, n_cols, P, out, parts=None):
    """J of rows [0, P) of the label-major device pool ``d_vals`` (leading
    dimension ``ld``, ``n_cols`` columns) under ``fit`` into the device vector
    ``out``.  ``parts``: a device tensor whose rows 0 and 1 (>= P long) receive
    log L_below and log L_above."""
    eng, dj, sets, sp = fit.eng, fit.dj, fit.sets, fit.sp
    t, lib = eng.torch, eng.lib
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


def sample_device(fit, seed, d_vals, ld, n_cols, row_base, n_rows, comp_out=None, comp_key=None):
    """Rows [row_base, row_base + n_rows) of the joint draw (module doc) from
    the below set of ``fit`` into rows [0, n_rows) of its labels' columns of
    the label-major device block ``d_vals`` (tpe_joint_sample).  ``comp_out``:
    a device int32 tensor for the rows' components; ``comp_key``: the component
    pick's key where it is not ``component_key(seed)`` (a group that is not
    the root's).  Three small uploads: the component cdf, the discrete labels'
    cdf table and the keys."""
    from . import tpe as T
    eng, dj, sp = fit.eng, fit.dj, fit.sp
    t, lib = eng.torch, eng.lib
    dset, n, _ = fit.sets[0]
    cdf = t.from_numpy(sample_cdf(n, fit.linear_forgetting, fit.prior_weight)).to(eng.device)
    cats = [np.cumsum(m.p) for m in dj.models if m.kind == _L.JOINT_CAT]
    cat_cdf = t.from_numpy(np.concatenate(cats)).to(eng.device) if cats else None
    keys = np.asarray([T.label_key(seed, m.label) for m in dj.models] +
                      [component_key(seed) if comp_key is None else comp_key], np.uint64)
    d_keys = t.from_numpy(keys.view(np.int64)).to(eng.device)
    _L.check(lib.tpe_joint_sample(dj.host.ctypes.data, dj.dev.data_ptr(), len(dj.models),
                                  dset.data_ptr(), n, cdf.data_ptr(),
                                  None if cat_cdf is None else cat_cdf.data_ptr(),
                                  0 if cat_cdf is None else cat_cdf.numel(), d_keys.data_ptr(),
                                  1.0 + float(fit.cat_smoothing), row_base, n_rows,
                                  d_vals.data_ptr(), ld, n_cols,
                                  None if comp_out is None else comp_out.data_ptr(), sp),
             "tpe_joint_sample")


def liar_device(fit, d_vals, ld, n_cols, P, S0, A0, taken, distinct, k, lie_weight, trace=False,
                rows_out=None):
    """The batch of module doc "Batches" for rows [0, P) of the label-major
    device pool ``d_vals``: the picks in order (numpy int64, at most k), all
    enqueued by one tpe_joint_lie_picks and read back once.  ``fit``: the
    joint labels' fit, whose above set lends its bandwidths; ``S0`` /
    ``A0``: device vectors (>= P doubles) of the score and of log L_above;
    ``taken`` / ``distinct``: device byte masks (``distinct`` may be None).
    None of them is written.  ``trace``: (rows, S_at_pick, S_k) as
    ``liar_numpy`` returns them.  ``rows_out``: a device int64 tensor of more
    than k entries to receive the rows (and, at entry k, their count) where the
    caller reads them on the device afterwards."""
    eng, dj, sp = fit.eng, fit.dj, fit.sp
    t, lib = eng.torch, eng.lib
    dset, n, _ = fit.sets[1]
    k = min(int(k), P)
    if k <= 0 or P == 0:
        none = np.zeros(0, np.int64)
        return (none, np.zeros(0), S0[:P].cpu().numpy()) if trace else none
    if n:  # (the prepared set's head: log w (n + 1), then sigma and 1 / (sqrt(2) sigma))
        sigma, sig_ptr = None, dset.data_ptr() + 8 * (n + 1)
    else:
        sig = lie_sigma(dj.models, 0, fit.bandwidth)
        some = sig > 0.0
        r = np.where(some, 1.0 / (math.sqrt(2.0) * np.where(some, sig, 1.0)), 0.0)
        sigma = t.from_numpy(np.concatenate([sig, r])).to(eng.device)
        sig_ptr = sigma.data_ptr()
    # the rows, then their count: one readback
    out = t.empty(k + 1, dtype=t.int64, device=eng.device) if rows_out is None else rows_out
    scratch = t.empty(lib.tpe_joint_lie_scratch_bytes(P), dtype=t.uint8, device=eng.device)
    at = t.empty(k, dtype=t.float64, device=eng.device) if trace else None
    S_k = t.empty(P, dtype=t.float64, device=eng.device) if trace else None
    _L.check(lib.tpe_joint_lie_picks(
        dj.host.ctypes.data, dj.dev.data_ptr(), len(dj.models),
        None if dj.tables is None else dj.tables.data_ptr(), dj.n_tables, sig_ptr,
        d_vals.data_ptr(), ld, n_cols, P, S0.data_ptr(), A0.data_ptr(),
        lie_log_total(n, fit.linear_forgetting, fit.prior_weight), math.log(lie_weight),
        taken.data_ptr(), None if distinct is None else distinct.data_ptr(), k, out.data_ptr(),
        out.data_ptr() + 8 * k, None if at is None else at.data_ptr(),
        None if S_k is None else S_k.data_ptr(), scratch.data_ptr(), sp), "tpe_joint_lie_picks")
    got = out[:k + 1].cpu().numpy()
    rows = got[:int(got[k])].copy()
    if not trace:
        return rows
    return rows, at.cpu().numpy()[:rows.size], S_k.cpu().numpy()


# -- groups on the device (module doc, "Groups") ---------------------------------
def sample_tree_device(fits, seed, d_vals, ld, n_cols, row_base, n_rows):
    """``sample_device`` per fit of ``fits`` (``fit(..., tree=True)``): every
    group's columns for all the rows, the root group under
    ``component_key(seed)``, the others under their ``group_component_key``."""
    for g, f in enumerate(fits):
        key = None if g == 0 else group_component_key(seed, f.group[0])
        sample_device(f, seed, d_vals, ld, n_cols, row_base, n_rows, comp_key=key)


def score_tree_device(fits, d_vals, d_active, ld, n_cols, P, out, parts=None):
    """S of ``joint="tree"`` for rows [0, P) of the label-major device pool
    ``d_vals`` / ``d_active`` (bytes; leading dimension ``ld``) under ``fits``
    (``fit(..., tree=True)``) into the device vector ``out``.  The root group
    goes through ``score_device`` (out = J_root: the flat case is that code
    alone).  Every other group, in order: the pool's rows in which the group is
    live compacted once into a device list (tpe_rows_compact on the first
    label's activity: a group's labels share theirs), then per window of
    ``ROWS_PER_CALL`` list positions log L_above into a dense temporary and
    log L_below minus it added to ``out`` at the listed rows
    (tpe_joint_score_rows).  The list's length never comes to the host.
    ``parts``: a (G, >= P) device tensor filled with NaN; row g receives J_g at
    the rows in which group g is live.

    ``fits`` of ``fit(..., tree="chain")``: S of ``joint="chain"``.  A fit with
    a context (``n_ctx`` > 0) takes tpe_joint_chain_rows in the same loop --
    log L - log L_ctx of the above set into the temporary, the below set's
    minus it added -- so row g of ``parts`` receives C_g; the list is still
    compacted on the group's first own label, not the context's."""
    eng = fits[0].eng
    t, lib = eng.torch, eng.lib
    score_device(fits[0], d_vals, ld, n_cols, P, out)
    if parts is not None:
        parts[0, :P].copy_(out[:P])
    if len(fits) == 1 or P == 0:
        return
    win = min(P, ROWS_PER_CALL)
    need = max((lib.tpe_joint_chain_scratch_bytes if f.n_ctx else lib.tpe_joint_scratch_bytes)
               (win, n) for f in fits[1:] for _, n, _ in f.sets)
    scratch = t.empty(max(need, 16), dtype=t.uint8, device=eng.device)
    above = t.empty(win, dtype=t.float64, device=eng.device)
    rows = t.empty(P, dtype=t.int64, device=eng.device)
    count = t.empty(1, dtype=t.int64, device=eng.device)
    cscratch = t.empty(lib.tpe_rows_compact_scratch_bytes(P), dtype=t.uint8, device=eng.device)
    both = _L.JOINT_OUT_SCATTER | _L.JOINT_OUT_ADD
    for g, f in enumerate(fits[1:], 1):
        dj, sets, sp = f.dj, f.sets, f.sp
        D = len(dj.models)
        tab = None if dj.tables is None else dj.tables.data_ptr()
        n_ctx = f.n_ctx
        flags = d_active.data_ptr() + dj.models[n_ctx].col * ld
        _L.check(lib.tpe_rows_compact(flags, P, rows.data_ptr(), count.data_ptr(),
                                      cscratch.data_ptr(), sp), "tpe_rows_compact")

        def score(which, p0, sub, dst, mode):
            dset, n, _ = sets[which]
            head = (dj.host.ctypes.data, dj.dev.data_ptr(), D)
            tail = (tab, dj.n_tables, dset.data_ptr(), n, d_vals.data_ptr(), ld, n_cols,
                    rows.data_ptr(), count.data_ptr(), p0, min(win, P - p0), sub, dst, mode,
                    scratch.data_ptr(), sp)
            if n_ctx:
                _L.check(lib.tpe_joint_chain_rows(*(head + (n_ctx,) + tail)),
                         "tpe_joint_chain_rows")
            else:
                _L.check(lib.tpe_joint_score_rows(*(head + tail)), "tpe_joint_score_rows")

        for p0 in range(0, P, win):
            score(1, p0, None, above.data_ptr(), 0)
            if parts is not None:  # (the same call as the one added to S: the same bits)
                score(0, p0, above.data_ptr(), parts[g].data_ptr(), _L.JOINT_OUT_SCATTER)
            score(0, p0, above.data_ptr(), out.data_ptr(), both)


# -- a grid pool: factor tables per axis ---------------------------
def score_grid_device(fits, pool, plan, d_axes, out, parts=None, tree=False):
    """The joint criterion of every row of the grid pool ``pool`` into the
    device vector ``out`` (>= len(pool) doubles), with the bits
    ``score_device`` / ``score_tree_device`` give the materialised pool.

    ``fits``: ``fit``'s result, one per group of the plan; ``plan``:
    ``pool.grid_joint_plan(pool, tree)``; ``d_axes``: the pool's concatenated
    axes on the device.  ``parts`` as the pool path takes it: a (3, >= P) tensor
    (log L_below, log L_above, J), or with ``tree`` a (G, >= P) tensor filled
    with NaN whose row g receives J_g where group g is live.

    Inside a component the factor a label adds depends on the label's value
    alone, so per set the factors of all axis values form a table F of
    (sum of the group's axis lengths) x C doubles (tpe_grid_joint_factors), and
    a row's a_i is log w_i plus one entry per label (tpe_grid_joint_score).

    Loop order.  Groups outermost, in group order (the root group stores S,
    every other group adds J_g).  Per group, a set whose whole F -- rounded up
    to whole chunks -- fits ``GRID_JOINT_TABLE_BYTES`` is built once, before
    any row; then blocks in which the group is live, in block order; then
    windows of at most ``GRID_ROWS_PER_CALL`` rows of the block; per window
    the above set into a temporary, then the below set minus it into ``out``.
    A set whose F is larger goes through one shared table of that many bytes
    in windows of whole chunks, inside the row window: rebuilt per row window
    and component window, scored into the scratch, merged after the last.
    Device memory: at most three tables of ``GRID_JOINT_TABLE_BYTES`` (both
    sets' and the shared one), 16 bytes of scratch per row of the window and
    chunk of the larger set, and 8 per row of the window."""
    eng = fits[0].eng
    t, lib = eng.torch, eng.lib
    chunk = lib.tpe_joint_chunk()
    P = len(pool)
    rows_max = max(b.rows for b in pool.blocks)
    win = min(rows_max, GRID_ROWS_PER_CALL)
    above = t.empty(win, dtype=t.float64, device=eng.device)
    n_axes = int(d_axes.numel())
    shared = None  # the table of the sets that do not fit one
    for g, f in enumerate(fits):
        dj, sets, sp = f.dj, f.sets, f.sp
        D = len(dj.models)
        cols = plan.groups[g]
        tab = None if dj.tables is None else dj.tables.data_ptr()
        axis_off = np.ascontiguousarray([pool.axis_off[j] for j in cols], np.int64)
        axis_len = np.ascontiguousarray([pool.axes[j].size for j in cols], np.int64)
        frow0 = np.ascontiguousarray([plan.axis_row[g][j] for j in cols], np.int64)
        n_frows = int(plan.n_frows[g])
        per = max(1, GRID_JOINT_TABLE_BYTES // (8 * chunk * n_frows))  # chunks per table
        need = max(lib.tpe_grid_joint_scratch_bytes(win, n) for _, n, _ in sets)
        scratch = t.empty(max(need, 16), dtype=t.uint8, device=eng.device)

        def factors(which, F, ldF, c0, nc):
            dset, n, _ = sets[which]
            _L.check(lib.tpe_grid_joint_factors(
                dj.host.ctypes.data, dj.dev.data_ptr(), D, tab, dj.n_tables, dset.data_ptr(), n,
                d_axes.data_ptr(), n_axes, axis_off.ctypes.data, axis_len.ctypes.data,
                frow0.ctypes.data, F.data_ptr(), ldF, n_frows, c0 * chunk, nc * chunk, sp),
                "tpe_grid_joint_factors")

        whole = []
        for which, (_dset, n, _) in enumerate(sets):
            chunks = (n + 1 + chunk - 1) // chunk
            F = None
            if chunks <= per:
                F = t.empty(n_frows * chunks * chunk, dtype=t.float64, device=eng.device)
                factors(which, F, chunks * chunk, 0, chunks)
            elif shared is None or shared.numel() < n_frows * per * chunk:
                shared = t.empty(n_frows * per * chunk, dtype=t.float64, device=eng.device)
            whole.append((F, chunks))

        def score(which, blk, r0, k, sub, dst, mode):
            dset, n, _ = sets[which]
            F, chunks = whole[which]
            step = chunks if F is not None else per
            for c0 in range(0, chunks, step):
                nc = min(step, chunks - c0)
                if F is None:
                    factors(which, shared, step * chunk, c0, nc)
                _L.check(lib.tpe_grid_joint_score(
                    (shared if F is None else F).data_ptr(), step * chunk, n_frows, c0 * chunk,
                    nc * chunk, dset.data_ptr(), n, blk.radix.ctypes.data,
                    blk.frow[g].ctypes.data, len(blk.radix), r0, k, sub, dst, mode,
                    scratch.data_ptr(), 1 if c0 + nc >= chunks else 0, sp),
                    "tpe_grid_joint_score")

        for b, blk in zip(pool.blocks, plan.blocks):
            if not blk.live[g]:
                continue
            for r0 in range(0, b.rows, win):
                k = min(win, b.rows - r0)
                at = 8 * (b.offset + r0)
                la = above.data_ptr()
                if parts is not None and not tree:
                    la = parts[1].data_ptr() + at
                score(1, blk, r0, k, None, la, _L.GRID_JOINT_STORE)
                if parts is not None and not tree:
                    score(0, blk, r0, k, None, parts[0].data_ptr() + at, _L.GRID_JOINT_STORE)
                if parts is not None and tree and g > 0:
                    # (the same call as the one added to S: the same bits)
                    score(0, blk, r0, k, la, parts[g].data_ptr() + at, _L.GRID_JOINT_STORE)
                score(0, blk, r0, k, la, out.data_ptr() + at,
                      _L.GRID_JOINT_ADD if g else _L.GRID_JOINT_STORE)
        if g == 0 and parts is not None:  # (J_root: S before anything is added to it)
            parts[0 if tree else 2, :P].copy_(out[:P])
