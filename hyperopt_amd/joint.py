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

The lie of ``batch="liar"`` acts through the always-live labels; on a
conditional space ``batch="liar-tree"`` ("Batches in a tree", below) lies inside
the branches as well.
``liar_numpy`` is this definition in numpy; ``liar_device`` enqueues all k
picks in one call (a pick's row is read on the device) and reads back the rows.

One engine, three entry modes.  This batch, "Batches in a tree" and "Batches in
a chain" (below) are a strict hierarchy: a flat space is a tree of one group
(the joint labels' fit, live in every row), a tree a chain whose contexts are
all empty.  The code has each thing once: ``_liar_numpy`` is the one pick loop
over a list of fits (``_lie_fits``), which ``liar_numpy``, ``liar_tree_numpy``
and ``liar_chain_numpy`` build for their mode; ``_liar_picks_device`` packs the
fits (``_lie_pack``) and makes the one call, tpe_joint_lie_chain_picks, for
``liar_device``, ``liar_tree_device`` and ``liar_chain_device``; and
csrc/tpe_joint_lie.hip holds one driver and one kernel pair behind the three C
entries.  The three model texts are the specification of their mode.

Chains (``joint="chain"``, csrc/tpe_joint.hip).  The
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

Refining (``refine=N``, csrc/tpe_joint_refine.hip).  Every path
above ends in an argmax over a finite set of rows, and the maximum of J lies
between them.  On the continuous labels J is smooth with a closed-form
gradient, so the picked rows are moved.  ``joint=True`` only.

  moving labels   a row's ``JOINT_CONT`` labels, D_c of them in list order, each
               in its fit coordinate t (log x for the log kinds).  Quantized and
               discrete labels, and every label under a ``switch``, stay.
               D_c == 0: the row is returned unchanged; D_c >
               ``TPE_REFINE_MAX_CONT`` (16): ValueError.
  evaluation   at a point t, per set: ``a_i`` of "Factors" / "Mixture", log L
               their log-sum-exp, ``r_i = exp(a_i - log L)``, ``dlogL_d = sum_i
               r_i (mu_{i,d} - t_d) / sigma_{i,d}^2`` (the set's bandwidth for a
               trial component, sigma_p for the prior; -log Z does not depend on
               t).  ``J(t) = log L_below - log L_above``, ``g_d = dlogL_below,d -
               dlogL_above,d``; a set with log L = -inf contributes no gradient.
  climb        evaluate at the start, h = 1; then ``refine`` times at the most,
               and only while h >= 2^-20: ``t'_d = clamp(t_d + (h s_d^2) g_d)``,
               s_d the below set's bandwidth of label d (sigma_p where that set
               is empty) -- with h = 1 and no above term the mean-shift (EM)
               step of the below mixture; ``clamp``, for a bounded kind, lifts
               to lo and cuts to nextafter(hi, -inf) (``draw64``'s rule).
               ``J(t') > J(t)``: t, J, g become those of t' and h = min(1, 2 h);
               otherwise, NaN on either side included, h = h / 2.
  result       a label whose t ends where it started keeps its stored bits;
               any other stores exp(t) for a log kind, else t.  J never
               decreases along the accepted points, ``refine=0`` is the identity
               bit for bit, and a row whose first J is NaN or +-inf is returned
               unchanged.  A row's result is a function of the row, the two
               sets and ``refine`` alone.

``refine_numpy`` is this definition in numpy; ``refine_device`` runs every
row's whole climb in one launch (inside a_i the device adds the fixed labels'
factors first, then the moving ones': its J equals the scorer's to rounding,
and ``tpe.refine_configs`` reports J before and after from ``score_device``).

Refining in a tree (``joint="tree"``, ``refine_tree=N``,
csrc/tpe_joint_refine_tree.hip).  On a space that opens with a
``switch`` every continuous label that matters sits inside a branch, where
``refine`` does not reach.  Under ``joint="tree"`` S(c) = sum_g J_g(c_g) over
disjoint label groups, so the climb separates exactly into one independent
climb per (row, live group).

  groups       those of ``joint_groups(domain)``, with the fits and sets of
               ``joint="tree"`` (``fit(..., tree=True)``).
  liveness     the root group is live in every row, group g > 0 where the
               ``active`` byte of its first label is set (the rule
               ``score_tree_device`` and ``liar_tree_*`` use).
  climb        for every row and every group g live in it, g's ``JOINT_CONT``
               labels -- D_c,g of them, in list order -- run the climb of
               "Refining", unchanged: with g's two sets, J_g, g's gradient, s_d
               from g's below set, and an h, decisions and 2^-20 stop of its
               own.  Quantized and discrete labels stay; the selectors are
               discrete, so liveness is constant along a climb.  Groups do not
               see each other.
  result       sum_g J_g never decreases; ``refine_tree=0`` is the identity bit
               for bit; a pair whose first J_g is NaN or +-inf does not move; a
               label that ends where it started keeps its stored bits; entries of
               labels not live in the row are never read or written.
  limits       D_c,g <= ``TPE_REFINE_MAX_CONT`` per group, G and D_tot <=
               ``TPE_COND_MAX_LABELS``; ValueError otherwise.
  identities   on a flat space (G = 1) the result has the bits of ``refine=N``
               with ``joint=True``; on any space the root group's columns have
               the bits ``refine=N`` / ``refine_configs`` give them, because the
               root fit is the ``joint=True`` fit.

``refine_tree_numpy`` is this definition in numpy (it and ``refine_numpy`` run
one helper, per mixture pair and row subset); ``refine_tree_device`` runs every
pair's whole climb in one tpe_joint_refine_tree, and
``tpe.refine_configs(joint="tree")`` reports J_g before and after from
``score_tree_device``'s per-group parts.

Bandwidth (``bandwidth="loo"``, ``tpe.joint_bandwidth``, csrc/tpe_joint_loo.hip,
DESIGN 3.5.11).  Every path above takes one multiplier h in ``sigma = h sigma_p
n ** (-1 / (D + 4))``; ``BANDWIDTH`` is a guess.  ``"loo"`` takes the grid value
that maximises the mixtures' leave-one-out log-likelihood on their own sets.

  set          a group's set of n rows in ascending row order, its label list
               ``models`` (D labels), ``sigma(h) = bandwidths(models, n, h)``, ``v =
               forgetting_weights(n, lf)``, ``W = sum(v) + prior_weight``.  Row i's
               x_i are its own stored history values, converted as a component's
               are (``randint``'s ``low`` comes off once, for rows and components
               alike).
  row          ``a_ij = log v_j + sum_d log k_{d,j}(x_{i,d})`` for every trial
               component j != i -- excluded by index: another trial with the same
               values stays in -- and ``a_i,prior = log prior_weight + sum_d log
               k_{d,prior}(x_{i,d})``; the factors are those of "Factors" with
               ``sigma(h)``.  ``LOO_i(h) = logsumexp(a_i.) - log(W - v_i)``.
  set score    ``Q_set(h) = sum_i v_i LOO_i(h) / sum_i v_i``; a set with n < 2 has
               Q_set = 0 for every h (nothing in it depends on h).
  choice       ``Q(h)`` = the sum of Q_set over the groups (``joint=True``: the
               joint labels' one group; ``"tree"``: those of ``joint_groups``),
               below set then above set.  The multiplier is the first grid value
               with the largest finite Q; ``BANDWIDTH`` where no set has n >= 2 or
               no Q is finite.
  grid         ascending, finite, > 0, 1 <= B <= ``TPE_LOO_MAX_GRID`` (16) values;
               the default ``LOO_GRID`` = BANDWIDTH 2^(k / 2), k = -6 .. 9.

``loo_numpy`` is this definition in numpy; ``loo_device`` runs one
tpe_joint_loo per set -- all B multipliers and all n^2 pairs in one call -- and
reads the (G, 2, B) curves back once.  ``bandwidth="loo"`` resolves the
multiplier once per public call, where the fit is made, over ``LOO_GRID``; the
float is what the fit, the lie, the climb and the settings hold from there on.

Bandwidth per label (``bandwidth="loo-label"``, ``tpe.joint_bandwidths``,
csrc/tpe_joint_loo_label.hip).  One h for every label lets the
labels the loss does not depend on take their share of the product kernel's
distance.  Here every label with a bandwidth (continuous or quantized) has its
own multiplier, chosen by the same likelihood, one coordinate at a time.

  multipliers  ``bandwidths(models, n, bandwidth)`` also takes a mapping label ->
               multiplier: ``sigma_d = h_d sigma_p,d n ** (-1 / (D + 4))``; a label
               the mapping does not name takes ``BANDWIDTH``, a discrete label has
               no bandwidth.  A float is unchanged bit for bit, and a mapping whose
               values all equal h gives the float's bits on every path: prep,
               score, tree, chain, draw, lie and refine read sigma through this
               function alone.
  curve        for a group's set (the sets, v, W, a_ij, LOO_i, Q_set and the n < 2
               rule of "Bandwidth"), current multipliers h, a label d with a
               bandwidth and a grid of B values: ``Q_set,d(b)`` = Q_set under
               sigma_e of h_e for e != d and sigma_d of ``grid[b]``.  ``Q_d(b)`` is
               the sum over the below and the above set of d's group; a label sits
               in exactly one group, so no other group depends on it.
  choice       start: every label at ``loo_choice`` over the same grid (what
               ``bandwidth="loo"`` returns); where that falls back -- no set with
               n >= 2, no finite Q -- every label gets ``BANDWIDTH`` and nothing
               else is run.  Then at most ``sweeps`` (default 2) passes over the
               groups in ``joint_groups`` order and their labels with a bandwidth
               in list order: label d keeps its value unless some grid value's Q_d
               is finite and strictly larger than Q_d at the current value, and
               then takes the first grid value with the largest finite Q_d.  An
               update is visible to the next label (Gauss-Seidel), so Q never
               falls along the run; a pass that changes nothing ends it.  Every
               multiplier returned is a grid value (``check_grid``'s rules).

``loo_label_numpy`` is the curve and ``loo_label_fit_numpy`` the run in numpy;
``loo_label_choice`` is the rule both it and the device path go through.
``loo_label_device`` runs ``loo_device`` for the start, then per visited label
two tpe_joint_loo_label calls (below set, above set) and one readback of the B
values: the choice is made on the host and steers the next call.
``bandwidth="loo-label"`` is resolved where ``"loo"`` is, into the mapping.

Batches in a tree (``joint="tree"``, ``batch="liar-tree"``,
csrc/tpe_joint_lie.hip).  Under ``joint="tree"`` every group
has an above mixture of its own, so a pick joins each one it is live in: two
rows equal at the root and different under a ``switch`` get different
penalties.  Groups g = 0 .. G - 1 are those of ``joint_groups(domain)``; the
root, g = 0, is live in every row, group g > 0 where the ``active`` byte of its
first label is set (the rule ``score_tree_device`` compacts on).

  inputs       ``S_0[r]``, the ``joint="tree"`` score, bits unchanged; ``A_g[r]
               = log L_above,g(r)`` for every (g, r) with g live in r -- the
               value the tree scoring subtracts for that row, read nowhere else.
               Per group: n_g the size of its prepared above set, ``sig_g =
               lie_sigma(models_g, n_g, bandwidth)``, ``log W_g =
               lie_log_total(n_g, lf, prior_weight)``.
  lie          pick p lies in every group g live in row p: ``c_{g,p}(r) =
               log(lie_weight) + sum_{d in g} log k_d(r_d)``, sequentially over
               g's labels in list order from ``log(lie_weight)``; ``log k_d`` is
               the "Factors" entry of a trial component of g's above set whose
               observation is row p's stored value, with ``sig_g`` -- the
               expressions of "Batches".  Defined for the rows in which g is live.
  update       ``U_{g,0}[r] = log W_g + A_g[r]``.  After pick j, for every g live
               in both p_j and r, ``U_{g,j}[r]`` is the join of ``U_{g,j-1}[r]``
               and ``c_{g,p_j}(r)`` by the "Batches" rule (U's term first; m =
               -inf gives -inf; c = -inf leaves U's bits).  Every other (g, r)
               keeps ``U_{g,j-1}[r]``.
  score        s = ``S_0[r]``; then, in group order over the groups live in r,
               ``s = s - (U_{g,j}[r] - U_{g,0}[r])`` where ``U_{g,0}[r]`` is
               finite.  A group no pick has touched subtracts exactly 0.0; a NaN
               ``S_0`` stays NaN.
  picks        the order, the masks, ``distinct`` and the stop of "Batches".  k =
               1 is the plain first row of the tree S, bit for bit; on a flat
               space (G = 1) the rows, ``S_at_pick`` and ``S_k`` have the bits of
               ``batch="liar"`` with ``joint=True``.

``liar_tree_numpy`` is this definition in numpy.  ``score_tree_device(above=)``
keeps A_g while it scores (row 0 is the root's subtrahend itself; a group's
dense temporary is copied to its rows by tpe_rows_scatter: the above set is not
scored twice and the list's length stays on the device), and
``liar_tree_device`` enqueues all k picks in one call.

Batches in a chain (``joint="chain"``, ``batch="liar-chain"``,
csrc/tpe_joint_lie.hip).  C_g is a ratio, but of one
mixture: a pending trial joins the above mixture of every chain fit it is live
in, and that mixture's context marginal is the same mixture with g's factors
dropped -- so the lie joins numerator and denominator, and one walk over the
fit's labels gives both contributions.

  groups       g = 0 .. G - 1 and their fits are those of ``fit(...,
               tree="chain")``: fit g covers the labels ``ctx(g) + g``, the
               ``n_ctx`` context labels first; the root has ``n_ctx = 0``, and so
               has any group with an empty context.  The root is live in every
               row, group g > 0 where the ``active`` byte of its first own label
               (``models[n_ctx]``) is set -- the rule ``score_tree_device``
               compacts on.  Where g is live, all of ctx(g) is (the definition
               of a context).
  inputs       ``S_0[r]``, the ``joint="chain"`` score, bits unchanged; ``A_g[r] =
               log L_above`` of fit g at row r for every (g, r) with g live in r,
               and ``B_g[r] = log L_ctx,above`` for the fits with ``n_ctx > 0``:
               the two values whose difference the chain scoring subtracts.  Per
               fit: n_g the size of its prepared above set, ``sig_g =
               lie_sigma(models_g, n_g, bandwidth)`` over all of ``ctx + g``,
               ``log W_g = lie_log_total(n_g, lf, prior_weight)``.
  lie          pick p lies in every g live in row p.  The walk runs over fit g's
               labels in list order from ``log(lie_weight)`` and adds ``log
               k_d(r_d)``, the "Factors" entry of a trial component whose
               observation is row p's stored value, with ``sig_g`` -- the
               expressions of "Batches".  The sum after the first ``n_ctx`` labels
               is ``c^ctx_{g,p}(r)``, the sum after all of them ``c_{g,p}(r)``.
  update       ``U_{g,0} = log W_g + A_g``, ``V_{g,0} = log W_g + B_g``.  After
               pick j, for every g live in both p_j and r, U joins ``c`` and V
               joins ``c^ctx`` by the "Batches" rule (the running term first; m =
               -inf gives -inf; c = -inf leaves the bits).  Every other (g, r)
               keeps its bits.
  score        s = ``S_0[r]``; then, in group order over the groups live in r: a
               group with ``n_ctx = 0`` gives ``s = s - (U_j - U_0)`` where U_0 is
               finite; one with ``n_ctx > 0`` gives ``s = s - ((U_j - U_0) - (V_j
               - V_0))`` where U_0 and V_0 are both finite, in that order of
               operations.  A group no pick has touched subtracts exactly 0.0; a
               NaN ``S_0`` stays NaN.
  picks        the order, the masks, ``distinct`` and the stop of "Batches".  k =
               1 is the first row of the chain S, bit for bit; a space whose
               groups all have empty contexts gives the rows, ``S_at_pick`` and
               ``S_k`` of ``batch="liar-tree"``, and a flat space those of
               ``batch="liar"``, bit for bit.

A group's penalty under ``"chain"`` is the change of a *conditional* log density,
and it may be negative: a row that shares the pick's context but lies far from it
inside g gains, because the pending trial raises the marginal at that context
more than the joint density there.  Over a row's groups the penalties sum to the
change of the log of the chain-rule above density -- the object a pending trial
in the history would change.

``liar_chain_numpy`` is this definition in numpy.  ``score_tree_device(above=,
above_ctx=)`` keeps A_g and B_g while it scores: a fit with a context writes both
from the merge that forms them (tpe_joint_chain_rows_keep; no scatter launch, the
above set is not scored twice), a fit without one fills ``above`` as under
``"tree"``.  ``liar_chain_device`` enqueues all k picks in one call.

Not built: a draw conditioned on the row's context (component weights ``w_i *
prod_ctx k``: ``joint="chain"`` draws as ``"tree"`` does).  ``joint="chain"``
on a ``GridPool`` (the factor tables hold one group's axes; a chain term needs
the context's as well).  A batch on a ``GridPool`` (a
grid has no row values to lie with) and under the factorised criterion (its
adaptive bandwidths depend on the sorted neighbours: no component can be added
without a refit).  ``refine`` / ``refine_tree`` under ``joint="chain"`` (a group's
term is a ratio over ctx + g: the groups are coupled through their contexts and
the climb does not separate).
``bandwidth="loo"`` / ``"loo-label"`` under ``joint="chain"`` (its fits are over
ctx + g and enter as a ratio: the likelihood of a set under its own fit is not
what they are ranked by) and on a ``GridPool`` (both take a float or a mapping).
Per-set multipliers (a label has one multiplier for its below and its above set).
"""
from __future__ import annotations

import ctypes
import math
from collections.abc import Mapping

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
    for a discrete label, and for n == 0: there is no such component).
    ``bandwidth``: one multiplier, or a mapping label -> multiplier (a label it
    does not name takes ``BANDWIDTH``)."""
    D = len(models)
    if isinstance(bandwidth, Mapping):  # (module doc, "Bandwidth per label")
        root = float(n) ** (-1.0 / (D + 4)) if n else 0.0
        return np.asarray([float(bandwidth.get(m.label, BANDWIDTH)) * root * m.sigma
                           for m in models])
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
        with np.errstate(invalid="ignore"):
            a = a + _label_term(m, hist, rows, sig[d], x[:, d], smoothing)
    return (_log_sum_exp(a), ctx) if n_ctx else _log_sum_exp(a)


def _label_term(m, hist, rows, sig_d, xd, smoothing):
    """log k of one label: the stored values ``xd`` (P,) under the n + 1
    components of the set of history rows ``rows``: (P, n + 1)."""
    n = rows.size
    obs = np.asarray(hist.vals)[rows, m.col] if n else np.zeros(0)
    if m.kind == _L.JOINT_CAT:
        hit, miss, prior = cat_tables(m, smoothing)
        c = np.rint(xd).astype(np.int64) - m.offset
        ci = np.rint(obs).astype(np.int64) - m.offset
        term = np.where(c[:, None] == ci[None, :], hit[c][:, None], miss[c][:, None])
        return np.concatenate([term, prior[c][:, None]], 1)
    mu = np.concatenate([_fit(m, obs), [m.mu]])
    sigma = np.concatenate([np.full(n, sig_d), [m.sigma]])
    return _density_terms(m, xd, mu, sigma)


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


def _lie_component(models, x, p, sig, smoothing, log_lie, start=None):
    """c_p(r) for every row r of ``x`` (P, D; stored values).  ``start``: the
    running sums to go on from in place of ``log_lie`` (a chain fit's own labels
    after its context's)."""
    c = np.full(x.shape[0], log_lie) if start is None else start
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


def _lie_join(u, c):
    """``u`` joined with ``c`` by the "Batches" rule, elementwise."""
    with np.errstate(all="ignore"):
        m = np.where(c > u, c, u)
        both = m + np.log(np.exp(u - m) + np.exp(c - m))
        return np.where(c == -np.inf, u, np.where(m == -np.inf, -np.inf, both))


def _lie_fits(domain, hist, vals, active, groups, gamma, lf, prior_weight, bandwidth):
    """The fits a batch lies in, for ``_liar_numpy``: per (labels, n_ctx) of
    ``groups`` (the root first; its rows are all live, a later fit's those where
    its first own label is active) the record (models, n_ctx, live rows, their
    stored values, sigma, log W)."""
    isa = split_sets(hist, gamma)[1]
    per = []
    for g, (labels, n_ctx) in enumerate(groups):
        models = label_models(domain, labels)
        cols = [m.col for m in models]
        live = np.flatnonzero(active[:, cols[n_ctx]]) if g else np.arange(vals.shape[0])
        n = int(set_rows(hist, isa, cols).size)
        per.append((models, n_ctx, live, vals[live][:, cols], lie_sigma(models, n, bandwidth),
                    lie_log_total(n, lf, prior_weight)))
    return per


def _log_lie(lie_weight):
    """log(lie_weight); ValueError unless it is > 0 and finite."""
    if not lie_weight > 0.0 or not np.isfinite(lie_weight):
        raise ValueError("lie_weight=%r must be > 0 and finite" % (lie_weight,))
    return math.log(lie_weight)


def _liar_numpy(per, S0, A, B, taken, distinct, k, log_lie, smoothing):
    """The pick loop of module doc "Batches in a chain" -- with every ``n_ctx``
    0 that of "Batches in a tree", with one fit that of "Batches" -- over the
    fits ``per`` (``_lie_fits``): (rows, S_at_pick, S_k, (U_0, U_k, V_0, V_k)),
    the state (P, G), NaN where nothing is kept.  ``A`` / ``B``: (P, G), ``B``
    read where a fit has a context."""
    S0 = np.asarray(S0, np.float64)
    P, G = S0.shape[0], len(per)
    A = np.asarray(A, np.float64).reshape(P, G)
    U0, V0 = np.full((P, G), np.nan), np.full((P, G), np.nan)
    for g, (_models, n_ctx, live, _x, _sig, log_w) in enumerate(per):
        U0[live, g] = log_w + A[live, g]
        if n_ctx:
            V0[live, g] = log_w + np.asarray(B, np.float64).reshape(P, G)[live, g]
    gone = np.zeros(P, bool)
    for mask in (taken, distinct):
        if mask is not None:
            gone |= np.asarray(mask)[:P] != 0
    U, V, S = U0.copy(), V0.copy(), S0.copy()
    rows, at = [], []
    for _ in range(min(max(int(k), 0), P)):
        p = _first_row(S, gone)
        if p < 0:
            break
        rows.append(p)
        at.append(S[p])
        gone[p] = True
        S = S0.copy()
        for g, (models, n_ctx, live, x, sig, _log_w) in enumerate(per):
            at_p = int(np.searchsorted(live, p))
            with np.errstate(all="ignore"):
                if at_p < live.size and live[at_p] == p:  # (g is live in the pick)
                    c = _lie_component(models[:n_ctx], x[:, :n_ctx], at_p, sig[:n_ctx],
                                       smoothing, log_lie)
                    if n_ctx:  # (the label boundary: c is c^ctx)
                        V[live, g] = _lie_join(V[live, g], c)
                    c = _lie_component(models[n_ctx:], x[:, n_ctx:], at_p, sig[n_ctx:],
                                       smoothing, log_lie, start=c)
                    U[live, g] = _lie_join(U[live, g], c)
                if n_ctx:
                    fin = live[np.isfinite(U0[live, g]) & np.isfinite(V0[live, g])]
                    S[fin] = S[fin] - ((U[fin, g] - U0[fin, g]) - (V[fin, g] - V0[fin, g]))
                else:
                    fin = live[np.isfinite(U0[live, g])]
                    S[fin] = S[fin] - (U[fin, g] - U0[fin, g])
    return np.asarray(rows, np.int64), np.asarray(at, np.float64), S, (U0, U, V0, V)


def liar_numpy(domain, hist, vals, k, taken=None, distinct=None, lie_weight=1.0, S0=None, A0=None,
               prior_weight=1.0, gamma=0.25, linear_forgetting=25, bandwidth=BANDWIDTH,
               cat_smoothing=CAT_SMOOTHING):
    """The batch of module doc "Batches" in numpy: (rows, S_at_pick, S_k) --
    the picks in order (int64, at most k), the score each was picked at, and
    the score of every row after the last pick.  ``vals``: (P, L) stored values
    as ``Pool.vals`` holds them; ``taken`` / ``distinct``: row masks (nonzero:
    not to be picked).  ``S0`` / ``A0``: the score and log L_above to start
    from where the caller has them (a device's, or S with the folded terms of
    a conditional space: the always-live labels alone lie); else
    ``score_numpy``'s J and log L_above."""
    domain, log_lie = as_domain(domain), _log_lie(lie_weight)
    vals = np.asarray(vals, np.float64)
    if S0 is None or A0 is None:
        J, _below, above = score_numpy(domain, hist, vals, None, prior_weight, gamma,
                                       linear_forgetting, bandwidth, cat_smoothing,
                                       return_parts=True)
        S0 = J if S0 is None else S0
        A0 = above if A0 is None else A0
    per = _lie_fits(domain, hist, vals, None, [(None, 0)], gamma, linear_forgetting, prior_weight,
                    bandwidth)
    return _liar_numpy(per, S0, A0, None, taken, distinct, k, log_lie, cat_smoothing)[:3]


def liar_tree_numpy(domain, hist, vals, k, active=None, taken=None, distinct=None,
                    lie_weight=1.0, S0=None, A=None, prior_weight=1.0, gamma=0.25,
                    linear_forgetting=25, bandwidth=BANDWIDTH, cat_smoothing=CAT_SMOOTHING):
    """The batch of module doc "Batches in a tree" in numpy: (rows, S_at_pick,
    S_k) as ``liar_numpy`` returns them.  ``vals`` / ``active``: (P, L) stored
    values and activity as a ``Pool`` holds them (``active`` None: where
    ``vals`` is not NaN).  ``S0`` (P,) / ``A`` (P, G; read where the group is
    live): the tree score and the groups' log L_above to start from where the
    caller has them; else ``score_numpy(tree=True)``'s."""
    domain, log_lie = as_domain(domain), _log_lie(lie_weight)
    vals = np.asarray(vals, np.float64)
    active = ~np.isnan(vals) if active is None else np.asarray(active, bool)
    if S0 is None or A is None:
        S, _J, _below, above = score_numpy(domain, hist, vals, active, prior_weight, gamma,
                                           linear_forgetting, bandwidth, cat_smoothing,
                                           return_parts=True, tree=True)
        S0 = S if S0 is None else S0
        A = above if A is None else A
    per = _lie_fits(domain, hist, vals, active, [(grp.labels, 0) for grp in joint_groups(domain)],
                    gamma, linear_forgetting, prior_weight, bandwidth)
    return _liar_numpy(per, S0, A, None, taken, distinct, k, log_lie, cat_smoothing)[:3]


def liar_chain_numpy(domain, hist, vals, k, active=None, taken=None, distinct=None,
                     lie_weight=1.0, S0=None, A=None, B=None, prior_weight=1.0, gamma=0.25,
                     linear_forgetting=25, bandwidth=BANDWIDTH, cat_smoothing=CAT_SMOOTHING,
                     return_state=False):
    """The batch of module doc "Batches in a chain" in numpy: (rows, S_at_pick,
    S_k) as ``liar_numpy`` returns them.  ``vals`` / ``active`` as
    ``liar_tree_numpy`` takes them.  ``S0`` (P,) / ``A`` / ``B`` (P, G; read where
    the group is live, ``B`` where it has a context too): the chain score and the
    fits' log L_above and log L_ctx,above to start from where the caller has
    them; else ``score_numpy(tree="chain")``'s.  ``return_state``: also (U_0,
    U_k, V_0, V_k), (P, G), NaN where nothing is kept."""
    domain, log_lie = as_domain(domain), _log_lie(lie_weight)
    vals = np.asarray(vals, np.float64)
    active = ~np.isnan(vals) if active is None else np.asarray(active, bool)
    if S0 is None or A is None or B is None:
        parts = score_numpy(domain, hist, vals, active, prior_weight, gamma, linear_forgetting,
                            bandwidth, cat_smoothing, return_parts=True, tree="chain")
        S0 = parts[0] if S0 is None else S0
        A = parts[3] if A is None else A
        B = parts[5] if B is None else B
    groups = [(ctx + grp.labels, len(ctx))
              for grp, ctx in zip(joint_groups(domain), joint_contexts(domain))]
    per = _lie_fits(domain, hist, vals, active, groups, gamma, linear_forgetting, prior_weight,
                    bandwidth)
    out = _liar_numpy(per, S0, A, B, taken, distinct, k, log_lie, cat_smoothing)
    return out[:3] + out[3] if return_state else out[:3]


# -- refining (module doc, "Refining") -------------------------------------------
REFINE_MIN_STEP = 2.0 ** -20
REFINE_TOL = 1e-6  # the project's relative tolerance per log-density (``info``'s bounds)


def check_refine(refine):
    """``refine`` as a step count: None is 0; ValueError for anything but a
    non-negative integer."""
    if refine is None:
        return 0
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or refine < 0:
        raise ValueError("refine=%r: None or an integer >= 0" % (refine,))
    return int(refine)


def moving_labels(models):
    """The positions in ``models`` of the labels a climb moves: the continuous
    ones, in list order (ValueError for more than ``REFINE_MAX_CONT``)."""
    cont = [d for d, m in enumerate(models) if m.kind == _L.JOINT_CONT]
    if len(cont) > _L.REFINE_MAX_CONT:
        raise ValueError("refine: %d continuous always-live labels, at most %d"
                         % (len(cont), _L.REFINE_MAX_CONT))
    return cont


def _refine_set(models, cont, hist, rows, x, t, lf, prior_weight, bandwidth, smoothing,
                bounds=False):
    """One set at the points ``t`` (P, D_c; fit coordinates of the labels
    ``cont``) of the rows ``x`` (P, D; stored values): log L (P,) and dlogL
    (P, D_c); then, zeros unless ``bounds`` (a check's, not the climb's): sum_i
    r_i |mu_i - t| / sigma_i^2 (P, D_c) and a bound K (P, D_c, D_c) on
    |d dlogL_d / d t_e|."""
    n, P, Dc = rows.size, x.shape[0], len(cont)
    a = np.broadcast_to(log_weights(n, lf, prior_weight), (P, n + 1)).copy()
    sig = bandwidths(models, n, bandwidth)
    pull = np.zeros((P, Dc, n + 1))  # (mu - t) / sigma^2
    curv = np.zeros((Dc, n + 1))  # 1 / sigma^2
    for d, m in enumerate(models):
        if m.kind == _L.JOINT_CONT:
            j = cont.index(d)
            obs = np.asarray(hist.vals)[rows, m.col] if n else np.zeros(0)
            mu = np.concatenate([_fit(m, obs), [m.mu]])
            sigma = np.concatenate([np.full(n, sig[d]), [m.sigma]])
            with np.errstate(all="ignore"):
                diff = t[:, j, None] - mu[None, :]
                z = diff / sigma[None, :]
                term = (-0.5 * z * z - np.log(sigma * math.sqrt(2.0 * math.pi)) +
                        _log_norm(m, mu, sigma))
                pull[:, j], curv[j] = -diff / sigma ** 2, 1.0 / sigma ** 2
        else:
            term = _label_term(m, hist, rows, sig[d], x[:, d], smoothing)
        with np.errstate(invalid="ignore"):
            a = a + term
    L = _log_sum_exp(a)
    with np.errstate(all="ignore"):
        r = np.where((L == -np.inf)[:, None], 0.0, np.exp(a - L[:, None]))  # (no pull)
        dlog = np.einsum("pc,pdc->pd", r, pull)
        if not bounds:
            return L, dlog, np.zeros((P, Dc)), np.zeros((P, Dc, Dc))
        m1 = np.einsum("pc,pdc->pd", r, np.abs(pull))
        # d/dt_e sum_i r_i pull_id = sum_i r_i pull_id (pull_ie - E pull_e) - [d == e] E 1/sigma^2
        K = (np.einsum("pc,pdc,pec->pde", r, np.abs(pull), np.abs(pull)) +
             m1[:, :, None] * m1[:, None, :])
        K[:, np.arange(Dc), np.arange(Dc)] += r @ curv.T
    return L, dlog, m1, K


def _refine_climb(models, sets, rows, hist, vals, refine, lf, prior_weight, bandwidth, smoothing,
                  return_info):
    """The climb of one mixture pair -- the labels ``models``, the two history
    row sets ``sets`` -- for the rows ``rows`` (indices) of ``vals``, written in
    place: (J_start, J_end, g_end, accepted, info or None) over those rows."""
    cont = moving_labels(models)
    cols = [m.col for m in models]
    rows = np.asarray(rows, np.int64)
    x = vals[np.ix_(rows, cols)]
    P, Dc = x.shape[0], len(cont)
    sb = bandwidths(models, sets[0].size, bandwidth)
    s2 = np.asarray([(sb[d] if sets[0].size else models[d].sigma) ** 2 for d in cont])
    t0 = np.stack([_fit(models[d], x[:, d]) for d in cont], 1) if Dc else np.zeros((P, 0))

    def evaluate(t):
        (Lb, db, ab, Kb), (La, da, aa, Ka) = [
            _refine_set(models, cont, hist, rows, x, t, lf, prior_weight, bandwidth,
                        smoothing, return_info) for rows in sets]
        with np.errstate(invalid="ignore"):
            return (Lb - La, db - da, REFINE_TOL * (np.abs(Lb) + np.abs(La)),
                    REFINE_TOL * (ab + aa), Kb + Ka)

    t = t0.copy()
    J, g, Jb, gb, K = evaluate(t)
    J_start = J.copy()
    # (the start itself: two implementations of log may differ in the last place)
    h, acc, tb = np.ones(P), np.zeros(P, np.int32), 4.0 * np.finfo(np.float64).eps * np.abs(t0)
    live = np.isfinite(J)
    margin = np.full((refine, P), np.nan)
    for it in range(refine):
        go = live & (h >= REFINE_MIN_STEP)
        if not go.any():
            break
        with np.errstate(all="ignore"):
            tt = t + (h[:, None] * s2[None, :]) * g
            for j, d in enumerate(cont):
                m = models[d]
                if m.bounded:  # (draw64's clamp)
                    tt[:, j] = np.where(tt[:, j] < m.lo, m.lo, tt[:, j])
                    tt[:, j] = np.where(tt[:, j] < m.hi, tt[:, j], np.nextafter(m.hi, -np.inf))
            Jn, gn, Jbn, gbn, Kn = evaluate(tt)
            better = go & (Jn > J)
        up = better[:, None]
        if return_info:  # (the bounds follow the climb; they never steer it)
            with np.errstate(all="ignore"):
                margin[it] = np.where(go, np.abs(Jn - J) / (Jbn + Jb), np.nan)
                # (a trial point that is the current point is a tie in any implementation)
                margin[it] = np.where(go & (tt == t).all(1), np.inf, margin[it])
                tbn = tb + (h[:, None] * s2[None, :]) * (np.einsum("pde,pe->pd", K, tb) + gb)
            gb, tb, Jb = np.where(up, gbn, gb), np.where(up, tbn, tb), np.where(better, Jbn, Jb)
            K = np.where(better[:, None, None], Kn, K)
        t, g, J = np.where(up, tt, t), np.where(up, gn, g), np.where(better, Jn, J)
        acc = acc + better.astype(np.int32)
        h = np.where(better, np.minimum(1.0, 2.0 * h), np.where(go, 0.5 * h, h))
    for j, d in enumerate(cont):  # (a label that did not move keeps its stored bits)
        moved = t[:, j] != t0[:, j]
        vals[rows[moved], cols[d]] = (np.exp(t[:, j]) if models[d].is_log else t[:, j])[moved]
    info = dict(J_bound=Jb, g_bound=gb, t_bound=tb, K=K, margin=margin) if return_info else None
    return J_start, J, g, acc, info


def refine_numpy(domain, hist, vals, refine, prior_weight=1.0, gamma=0.25, linear_forgetting=25,
                 bandwidth=BANDWIDTH, cat_smoothing=CAT_SMOOTHING, return_info=False):
    """The climb of module doc "Refining" in vectorised numpy, every row of
    ``vals`` ((P, L) stored values as ``Pool.vals`` holds them) by itself:
    (refined copy of ``vals``, J_start, J_end, g_end (P, D_c), accepted).

    ``return_info``: one more entry, what a comparison at ``REFINE_TOL`` per
    log-density needs, all from this reference alone: ``J_bound`` (P,) =
    tol (|log L_below| + |log L_above|) and ``g_bound`` (P, D_c) = tol sum_i
    r_i |mu_i - t| / sigma_i^2 over both sets, both at the last accepted point;
    ``t_bound`` (P, D_c), the bound on t there propagated per accepted step --
    a deviation dt of the point and dg <= g_bound of its gradient give
    dt'_d <= dt_d + h s_d^2 (sum_e K_de dt_e + dg_d), K bounding the gradient's
    derivative (``K`` (P, D_c, D_c), at the last accepted point; the clamp does
    not stretch a deviation); and ``margin`` (steps, P), per decision |J(t') -
    J(t)| over the sum of the two points' J bounds -- NaN where the row took no
    decision, inf where t' is t itself."""
    domain = as_domain(domain)
    refine = check_refine(refine)
    models = label_models(domain)
    moving_labels(models)  # (ValueError over the limit, before anything else)
    vals = np.array(vals, np.float64, ndmin=2)
    cols = [m.col for m in models]
    sets = [set_rows(hist, mask, cols) for mask in split_sets(hist, gamma)]
    out = _refine_climb(models, sets, np.arange(vals.shape[0]), hist, vals, refine,
                        linear_forgetting, prior_weight, bandwidth, cat_smoothing, return_info)
    return (vals,) + out[:4] + ((out[4],) if return_info else ())


def refine_tree_numpy(domain, hist, vals, refine, active=None, prior_weight=1.0, gamma=0.25,
                      linear_forgetting=25, bandwidth=BANDWIDTH, cat_smoothing=CAT_SMOOTHING,
                      return_info=False):
    """The climb of module doc "Refining in a tree" in numpy: every (row, live
    group) of ``vals`` by itself.  ``active`` ((P, L); None: where ``vals`` is
    not NaN) says where a group is live, by its first label.  Returns (refined
    copy of ``vals``, J_start (P, G), J_end (P, G), g_end (P, sum of D_c,g; group
    g's moving labels at the offset of the groups before it), accepted (P, G)),
    NaN / 0 where a group is not live.  ``return_info``: one more entry,
    ``refine_numpy``'s dict with the same shapes -- ``J_bound`` (P, G),
    ``g_bound`` / ``t_bound`` (P, sum D_c,g), ``K`` a list per group of (P,
    D_c,g, D_c,g) (NaN rows where it is not live) and ``margin`` (steps, P, G)."""
    domain = as_domain(domain)
    refine = check_refine(refine)
    groups = [label_models(domain, grp.labels) for grp in joint_groups(domain)]
    Dc = [len(moving_labels(models)) for models in groups]
    check_tree_limits(groups)
    vals = np.array(vals, np.float64, ndmin=2)
    active = ~np.isnan(vals) if active is None else np.asarray(active, bool)
    P, G, off = vals.shape[0], len(groups), np.concatenate([[0], np.cumsum(Dc)]).astype(int)
    J0, J1 = np.full((P, G), np.nan), np.full((P, G), np.nan)
    g_end, acc = np.full((P, off[-1]), np.nan), np.zeros((P, G), np.int32)
    info = dict(J_bound=np.full((P, G), np.nan), g_bound=np.full((P, off[-1]), np.nan),
                t_bound=np.full((P, off[-1]), np.nan), K=[],
                margin=np.full((refine, P, G), np.nan))
    masks = split_sets(hist, gamma)
    for g, models in enumerate(groups):
        cols = [m.col for m in models]
        rows = np.arange(P) if g == 0 else np.flatnonzero(active[:, cols[0]])
        sets = [set_rows(hist, mask, cols) for mask in masks]
        a, b, c, d, more = _refine_climb(models, sets, rows, hist, vals, refine,
                                         linear_forgetting, prior_weight, bandwidth,
                                         cat_smoothing, return_info)
        sl = slice(off[g], off[g + 1])
        J0[rows, g], J1[rows, g], g_end[rows, sl], acc[rows, g] = a, b, c, d
        if return_info:
            for name in ("J_bound", "g_bound", "t_bound"):
                info[name][rows, sl if name != "J_bound" else g] = more[name]
            K = np.full((P, Dc[g], Dc[g]), np.nan)
            K[rows] = more["K"]
            info["K"].append(K)
            info["margin"][:, rows, g] = more["margin"]
    out = (vals, J0, J1, g_end, acc)
    return out + (info,) if return_info else out


def check_tree_limits(groups):
    """ValueError where tpe_joint_refine_tree would return TPE_E_UNSUPPORTED:
    more than ``COND_MAX_LABELS`` groups, or labels over all of them (``groups``:
    one label-model list per group; ``moving_labels`` checks a group's D_c)."""
    G, D_tot = len(groups), sum(len(models) for models in groups)
    if G > _L.COND_MAX_LABELS or D_tot > _L.COND_MAX_LABELS:
        raise ValueError("refine_tree: %d groups of %d labels in all, at most %d of either"
                         % (G, D_tot, _L.COND_MAX_LABELS))


# -- bandwidth (module doc, "Bandwidth") -----------------------------------------
LOO_GRID = BANDWIDTH * 2.0 ** (np.arange(-6, 10) / 2.0)
LOO_BAD_GRID = ("a bandwidth grid is 1 to %d multipliers: ascending, finite, > 0"
                % _L.LOO_MAX_GRID)
LOO_CHAIN = ("bandwidth='loo' is not built for joint='chain': its fits are over ctx + g and "
             "enter as a ratio (joint.py, \"Not built\"); joint=True or joint='tree'")
LOO_GRID_POOL = ("bandwidth='loo' is not built for a GridPool (joint.py, \"Not built\"): pass the "
                 "float of tpe.joint_bandwidth(domain, trials)")


def check_grid(grid):
    """``grid`` as a float64 vector (None: ``LOO_GRID``); ValueError(LOO_BAD_GRID)."""
    if grid is None:
        return LOO_GRID.copy()
    try:
        grid = np.array(grid, np.float64, ndmin=1)
    except (TypeError, ValueError):
        raise ValueError(LOO_BAD_GRID)
    if (grid.ndim != 1 or not 1 <= grid.size <= _L.LOO_MAX_GRID or
            not (np.isfinite(grid) & (grid > 0.0)).all() or not (np.diff(grid) > 0.0).all()):
        raise ValueError(LOO_BAD_GRID)
    return grid


def loo_sets(domain, hist, gamma, tree=False):
    """[(models, [below rows, above rows])] per group the likelihood covers:
    the joint labels' one group, or with ``tree`` those of ``joint_groups``."""
    domain = as_domain(domain)
    if tree == "chain":
        raise ValueError(LOO_CHAIN)
    groups = [grp.labels for grp in joint_groups(domain)] if tree else [None]
    masks = split_sets(hist, gamma)
    out = []
    for group in groups:
        models = label_models(domain, group)
        cols = [m.col for m in models]
        out.append((models, [set_rows(hist, mask, cols) for mask in masks]))
    return out


def _loo_set(models, hist, rows, sigmas, lf, prior_weight, smoothing):
    """Q_set of the set of history rows ``rows`` under each row of ``sigmas``
    ((B, D): the trial components' sigma per label): (B,)."""
    n = rows.size
    if n < 2:
        return np.zeros(len(sigmas))
    v = forgetting_weights(n, lf)
    W = v.sum() + float(prior_weight)
    x = np.asarray(hist.vals)[rows]
    own = np.arange(n)
    Q = np.zeros(len(sigmas))
    for b, sig in enumerate(sigmas):
        with np.errstate(divide="ignore"):
            a = np.broadcast_to(np.log(np.concatenate([v, [float(prior_weight)]])),
                                (n, n + 1)).copy()
        for d, m in enumerate(models):
            with np.errstate(invalid="ignore"):
                a = a + _label_term(m, hist, rows, sig[d], x[:, m.col], smoothing)
        a[own, own] = -np.inf  # (itself, by index)
        with np.errstate(all="ignore"):
            Q[b] = (v * (_log_sum_exp(a) - np.log(W - v))).sum() / v.sum()
    return Q


def loo_numpy(domain, hist, grid=None, tree=False, prior_weight=1.0, gamma=0.25,
              linear_forgetting=25, cat_smoothing=CAT_SMOOTHING):
    """Q_set (module doc, "Bandwidth") of every group's below and above set over
    the multipliers ``grid``, in vectorised numpy: fp64 (G, 2, B)."""
    grid = check_grid(grid)
    return np.asarray([[_loo_set(models, hist, rows,
                                 [bandwidths(models, rows.size, h) for h in grid],
                                 linear_forgetting, prior_weight, cat_smoothing) for rows in sets]
                       for models, sets in loo_sets(domain, hist, gamma, tree)])


def _loo_argmax(grid, Q_sets, sizes):
    """The index ``loo_choice`` takes, or None where it falls back."""
    with np.errstate(invalid="ignore"):
        Q = np.asarray(Q_sets, np.float64).sum((0, 1))
    fin = np.isfinite(Q)
    if not (np.asarray(sizes) >= 2).any() or not fin.any():
        return None
    return int(np.argmax(np.where(fin, Q, -np.inf)))


def loo_choice(grid, Q_sets, sizes):
    """The multiplier of module doc "Bandwidth": ``Q_sets`` (G, 2, B) summed
    over the sets, the first grid value with the largest finite sum;
    ``BANDWIDTH`` where no set of ``sizes`` (the sets' n) reaches 2 or no sum
    is finite."""
    b = _loo_argmax(grid, Q_sets, sizes)
    return BANDWIDTH if b is None else float(np.asarray(grid)[b])


# -- bandwidth per label (module doc, "Bandwidth per label") -----------------------
def check_sweeps(sweeps):
    """``sweeps`` as an int >= 0, else ValueError."""
    if isinstance(sweeps, bool) or not isinstance(sweeps, (int, np.integer)) or sweeps < 0:
        raise ValueError("sweeps=%r: an integer >= 0" % (sweeps,))
    return int(sweeps)


def check_bandwidth_map(bandwidth, labels=None):
    """A mapping label -> multiplier as a dict of floats; ValueError on a key
    that is not one of ``labels`` (None: not checked) and on a value that is
    not a finite number > 0."""
    out = {}
    for lab, h in bandwidth.items():
        if labels is not None and lab not in labels:
            raise ValueError("bandwidth: %r is not a label of the space" % (lab,))
        try:
            h = float(h)
        except (TypeError, ValueError):
            raise ValueError("bandwidth[%r]=%r: a finite number > 0" % (lab, h))
        if not (h > 0.0 and math.isfinite(h)):
            raise ValueError("bandwidth[%r]=%r: a finite number > 0" % (lab, h))
        out[lab] = h
    return out


def bandwidth_key(bandwidth):
    """``bandwidth`` as it enters a comparison or a key: a mapping as the sorted
    tuple of its items, anything else as it is."""
    return tuple(sorted(bandwidth.items())) if isinstance(bandwidth, Mapping) else bandwidth


def banded_labels(sets):
    """The labels with a bandwidth (continuous or quantized) of ``loo_sets``'s
    groups, in the order the sweeps visit them: [(group index, label index in
    the group, label)]."""
    return [(g, d, m.label) for g, (models, _pair) in enumerate(sets)
            for d, m in enumerate(models) if m.kind != _L.JOINT_CAT]


def loo_label_numpy(domain, hist, mult, label, grid=None, tree=False, prior_weight=1.0,
                    gamma=0.25, linear_forgetting=25, cat_smoothing=CAT_SMOOTHING):
    """Q_set,d (module doc, "Bandwidth per label") of the below and the above
    set of ``label``'s group, ``label`` over ``grid`` and every other label at
    its multiplier of the mapping ``mult``: fp64 (2, B)."""
    grid = check_grid(grid)
    sets = loo_sets(domain, hist, gamma, tree)
    where = [(g, d) for g, d, lab in banded_labels(sets) if lab == label]
    if not where:
        raise ValueError("%r is not a label with a bandwidth of the joint criterion" % (label,))
    (g, d), out = where[0], []
    models, pair = sets[g]
    for rows in pair:
        sig = np.tile(bandwidths(models, rows.size, mult), (grid.size, 1))
        sig[:, d] = [bandwidths(models, rows.size, h)[d] for h in grid]
        out.append(_loo_set(models, hist, rows, sig, linear_forgetting, prior_weight,
                            cat_smoothing))
    return np.asarray(out)


def loo_label_choice(grid, Q_sets, sizes, labels, curve, sweeps=2):
    """The multipliers of module doc "Bandwidth per label": (mapping, visited).
    ``Q_sets`` / ``sizes``: the scalar curves and set sizes ``loo_choice``
    takes, for the start; ``labels``: the labels with a bandwidth in visiting
    order; ``curve(mult, label)`` -> (2, B), Q_set,d of the label's below and
    above set under the mapping ``mult``; ``visited``: [(label, curve)] in the
    order the run asked for them."""
    grid, sweeps = np.asarray(grid, np.float64), check_sweeps(sweeps)
    start = _loo_argmax(grid, Q_sets, sizes)
    if start is None:
        return {lab: BANDWIDTH for lab in labels}, []
    at = {lab: start for lab in labels}
    mult = {lab: float(grid[start]) for lab in labels}
    visited = []
    for _sweep in range(sweeps):
        moved = False
        for lab in labels:
            Q2 = np.asarray(curve(dict(mult), lab), np.float64)
            visited.append((lab, Q2))
            with np.errstate(invalid="ignore"):
                Q = Q2.sum(0)
            fin = np.isfinite(Q)
            if not fin.any():
                continue
            best = int(np.argmax(np.where(fin, Q, -np.inf)))
            if Q[best] > Q[at[lab]]:  # (strictly: a tie keeps the value)
                at[lab], mult[lab], moved = best, float(grid[best]), True
        if not moved:
            break
    return mult, visited


def loo_label_fit_numpy(domain, hist, grid=None, tree=False, sweeps=2, prior_weight=1.0,
                        gamma=0.25, linear_forgetting=25, cat_smoothing=CAT_SMOOTHING):
    """``loo_label_choice`` over ``loo_numpy`` and ``loo_label_numpy``:
    (mapping, visited)."""
    grid = check_grid(grid)
    kw = dict(prior_weight=prior_weight, gamma=gamma, linear_forgetting=linear_forgetting,
              cat_smoothing=cat_smoothing)
    sets = loo_sets(domain, hist, gamma, tree)
    sizes = [[rows.size for rows in pair] for _m, pair in sets]
    return loo_label_choice(
        grid, loo_numpy(domain, hist, grid, tree, **kw), sizes,
        [lab for _g, _d, lab in banded_labels(sets)],
        lambda mult, lab: loo_label_numpy(domain, hist, mult, lab, grid, tree, **kw), sweeps)


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


def _inv_sqrt2_sigma(sig):
    """1 / (sqrt(2) sigma) per entry of ``sig``, and 0 where sigma is 0 (a
    discrete label, and every label of an empty set, has no bandwidth: never an
    infinity)."""
    some = sig > 0.0
    return np.where(some, 1.0 / (math.sqrt(2.0) * np.where(some, sig, 1.0)), 0.0)


def _prepare_set(eng, dj, seen, hist_cols, rows, lf, prior_weight, bandwidth, sp):
    """One set on the device: (set tensor, n, row list).  ``seen``: the history
    on the device (``fit``); ``rows``: the set's rows as rows of that mirror."""
    t, lib = eng.torch, eng.lib
    _alive, sv, sa, sld, _srows, _n = seen
    D, n = len(dj.models), int(rows.size)
    sig = bandwidths(dj.models, n, bandwidth)
    head = np.concatenate([log_weights(n, lf, prior_weight), sig, _inv_sqrt2_sigma(sig)])
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
                 "linear_forgetting", "bandwidth", "cat_smoothing", "lie_pack")


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
        f.eng, f.group, f.n_ctx, f.lie_pack = eng, group, len(ctx), None
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


def _score_fit(fit, d_vals, ld, n_cols, P, out, listed=None, above_to=None, ctx_to=None,
               below_to=None, j_to=None):
    """J of one fit, per window of ``ROWS_PER_CALL`` rows: the above set's value
    into a temporary, the below set's minus it into ``out``.

    Dense (``listed`` None): rows [0, P) by tpe_joint_score, ``out[r]`` = J.
    ``above_to``: a device vector (>= P) that takes the temporary's place, so
    log L_above stays; ``below_to``: a device vector (>= P) that receives log
    L_below, by one more call.

    ``listed`` = (rows, count), a device list of pool rows and its length:
    windows of list positions by tpe_joint_score_rows, J added to ``out`` at
    the listed rows; a fit with a context takes tpe_joint_chain_rows, and J is
    C_g.  ``j_to``: a device vector that receives J itself at the listed rows,
    by one more call.  ``above_to`` receives log L_above at the listed rows: the
    temporary by one tpe_rows_scatter per window, or with a context from the
    merge that forms it (tpe_joint_chain_rows_keep), which leaves log L_ctx,above
    in ``ctx_to`` where that is given."""
    eng, dj, sets, sp, n_ctx = fit.eng, fit.dj, fit.sets, fit.sp, fit.n_ctx
    t, lib = eng.torch, eng.lib
    labels = (dj.host.ctypes.data, dj.dev.data_ptr(), len(dj.models))
    pool = (d_vals.data_ptr(), ld, n_cols)
    tab = None if dj.tables is None else dj.tables.data_ptr()
    win = min(max(P, 1), ROWS_PER_CALL)
    size = lib.tpe_joint_chain_scratch_bytes if n_ctx else lib.tpe_joint_scratch_bytes
    scratch = t.empty(max(max(size(win, n) for _, n, _ in sets), 16), dtype=t.uint8,
                      device=eng.device)
    dense_to = None if listed is not None else above_to
    temp = t.empty(win, dtype=t.float64, device=eng.device) if dense_to is None else None
    lst = () if listed is None else (listed[0].data_ptr(), listed[1].data_ptr())
    end = (scratch.data_ptr(), sp)
    kept = None
    if lst and n_ctx and above_to is not None:
        # (the kept vectors' common length: no row past either is written)
        kept = (above_to.data_ptr(), None if ctx_to is None else ctx_to.data_ptr(),
                min(v.shape[0] for v in (above_to, ctx_to) if v is not None))

    def score(which, r0, sub, dst, mode=0, keep=None):
        dset, n, _ = sets[which]
        data = (tab, dj.n_tables, dset.data_ptr(), n) + pool + lst + (r0, min(win, P - r0), sub, dst)
        if not lst:
            _L.check(lib.tpe_joint_score(*labels, *data, *end), "tpe_joint_score")
        elif not n_ctx:
            _L.check(lib.tpe_joint_score_rows(*labels, *data, mode, *end), "tpe_joint_score_rows")
        elif keep is None:
            _L.check(lib.tpe_joint_chain_rows(*labels, n_ctx, *data, mode, *end),
                     "tpe_joint_chain_rows")
        else:  # (the two values the merge subtracts stay)
            _L.check(lib.tpe_joint_chain_rows_keep(*labels, n_ctx, *data, mode, *keep, *end),
                     "tpe_joint_chain_rows_keep")

    for r0 in range(0, P, win):
        # above first: the below call subtracts it
        la = temp.data_ptr() if dense_to is None else dense_to.data_ptr() + 8 * r0
        score(1, r0, None, la, keep=kept)
        if not lst:
            if below_to is not None:
                # log L_below by itself costs one more call: J keeps the bits of the
                # call without it because it is made by the same call
                score(0, r0, None, below_to.data_ptr() + 8 * r0)
            score(0, r0, la, out.data_ptr() + 8 * r0)
            continue
        if above_to is not None and kept is None:
            _L.check(lib.tpe_rows_scatter(la, *lst, r0, min(win, P - r0), above_to.data_ptr(),
                                          above_to.shape[0], sp), "tpe_rows_scatter")
        if j_to is not None:  # (the same call as the one added to S: the same bits)
            score(0, r0, la, j_to.data_ptr(), _L.JOINT_OUT_SCATTER)
        score(0, r0, la, out.data_ptr(), _L.JOINT_OUT_SCATTER | _L.JOINT_OUT_ADD)


def score_device(fit, d_vals, ld, n_cols, P, out, parts=None, keep_above=None):
    """J of rows [0, P) of the label-major device pool ``d_vals`` (leading
    dimension ``ld``, ``n_cols`` columns) under ``fit`` into the device vector
    ``out``.  ``parts``: a device tensor whose rows 0 and 1 (>= P long) receive
    log L_below and log L_above.  ``keep_above`` (without ``parts``): a device
    vector (>= P doubles) that takes the temporary's place, so log L_above stays
    -- the same calls."""
    if parts is not None:
        _score_fit(fit, d_vals, ld, n_cols, P, out, above_to=parts[1], below_to=parts[0])
    else:
        _score_fit(fit, d_vals, ld, n_cols, P, out, above_to=keep_above)


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


class _LiePack(object):
    """The fits of a batch as tpe_joint_lie_chain_picks takes them: the label
    records concatenated in fit order (``tab_off`` counted from the start of the
    concatenated tables) on the host and on the device, the tables,
    ``group_off``, log W_g, ``n_ctx`` (a fit's records are its context's, then
    its own), the liveness columns (the first own label's; -1 for the root),
    the sigmas, and ``fits`` itself."""
    __slots__ = ("fits", "host", "dev", "tables", "n_tables", "off", "log_w", "col", "sigma",
                 "n_ctx")


def _lie_pack(fits):
    """``_LiePack`` of ``fits`` (``fit``'s list, or the joint labels' fit
    alone), made once per fit list and kept on its first fit."""
    pk = fits[0].lie_pack
    if pk is not None and pk.fits == list(fits):  # (a JointFit equals itself alone)
        return pk
    eng = fits[0].eng
    t = eng.torch
    recs, tabs, sig, off, base = [], [], [], [0], 0
    for f in fits:
        rec = f.dj.host.copy()
        rec["tab_off"][rec["kind"] == _L.JOINT_CAT] += base
        recs.append(rec)
        if f.dj.tables is not None:
            tabs.append(f.dj.tables)
        base += f.dj.n_tables
        off.append(off[-1] + len(f.dj.models))
        sig.append(lie_sigma(f.dj.models, f.sets[1][1], f.bandwidth))
    sig = np.concatenate(sig)
    pk = _LiePack()
    pk.fits = list(fits)
    pk.host = np.concatenate(recs)
    pk.dev = t.from_numpy(pk.host.view(np.uint8).copy()).to(eng.device)
    pk.tables, pk.n_tables = (t.cat(tabs) if tabs else None), base
    pk.off = np.asarray(off, np.int32)
    pk.log_w = np.asarray([lie_log_total(f.sets[1][1], f.linear_forgetting, f.prior_weight)
                           for f in fits], np.float64)
    pk.n_ctx = np.asarray([f.n_ctx for f in fits], np.int32)
    pk.col = np.asarray([-1] + [f.dj.models[f.n_ctx].col for f in fits[1:]], np.int32)
    # (no label with a bandwidth: the call takes no sigmas)
    pk.sigma = (t.from_numpy(np.concatenate([sig, _inv_sqrt2_sigma(sig)])).to(eng.device)
                if (sig > 0.0).any() else None)
    fits[0].lie_pack = pk
    return pk


def _liar_picks_device(fits, d_vals, d_active, ld, n_cols, P, S0, A, B, taken, distinct, k,
                       lie_weight, trace, rows_out):
    """The k picks of a batch over ``fits`` for rows [0, P) of the label-major
    device pool ``d_vals`` / ``d_active``: the picks in order (numpy int64, at
    most k), all enqueued by one tpe_joint_lie_chain_picks -- the joint labels'
    fit alone is its G = 1, tree fits are its fits without a context -- and read
    back once.  ``S0``: the score, a device vector (>= P doubles); ``A`` / ``B``:
    log L_above and log L_ctx,above per fit, (G, >= P) (one fit: a vector; ``B``
    is read where a fit has a context); ``taken`` / ``distinct``: device byte
    masks (``distinct`` may be None).  None of them is written.  ``trace``:
    (rows, S_at_pick, S_k) as ``liar_numpy`` returns them.  ``rows_out``: a
    device int64 tensor of more than k entries to receive the rows (and, at
    entry k, their count) where the caller reads them on the device afterwards."""
    eng, sp = fits[0].eng, fits[0].sp
    t, lib = eng.torch, eng.lib
    k = min(int(k), P)
    if k <= 0 or P == 0:
        none = np.zeros(0, np.int64)
        return (none, np.zeros(0), S0[:P].cpu().numpy()) if trace else none
    pk = _lie_pack(fits)
    G, n_v = len(fits), int((pk.n_ctx > 0).sum())
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    # the rows, then their count: one readback
    out = t.empty(k + 1, dtype=t.int64, device=eng.device) if rows_out is None else rows_out
    scratch = t.empty(lib.tpe_joint_lie_chain_scratch_bytes(P, G, n_v), dtype=t.uint8,
                      device=eng.device)
    at = t.empty(k, dtype=t.float64, device=eng.device) if trace else None
    S_k = t.empty(P, dtype=t.float64, device=eng.device) if trace else None
    _L.check(lib.tpe_joint_lie_chain_picks(
        pk.host.ctypes.data, pk.dev.data_ptr(), len(pk.host), ptr(pk.tables), pk.n_tables,
        pk.off.ctypes.data, pk.log_w.ctypes.data, pk.col.ctypes.data, pk.n_ctx.ctypes.data, G,
        ptr(pk.sigma), d_vals.data_ptr(), ptr(d_active), ld, n_cols, P, S0.data_ptr(),
        A.data_ptr(), A.shape[-1], ptr(B) if n_v else None, B.shape[-1] if n_v else 0,
        math.log(lie_weight), taken.data_ptr(), ptr(distinct), k, out.data_ptr(),
        out.data_ptr() + 8 * k, ptr(at), ptr(S_k), scratch.data_ptr(), sp),
        "tpe_joint_lie_chain_picks")
    got = out[:k + 1].cpu().numpy()
    rows = got[:int(got[k])].copy()
    if not trace:
        return rows
    return rows, at.cpu().numpy()[:rows.size], S_k.cpu().numpy()


def liar_device(fit, d_vals, ld, n_cols, P, S0, A0, taken, distinct, k, lie_weight, trace=False,
                rows_out=None):
    """The batch of module doc "Batches": ``_liar_picks_device`` over ``fit``
    alone, the joint labels' fit, whose above set lends its bandwidths; ``A0``: a
    device vector (>= P doubles) of log L_above."""
    return _liar_picks_device([fit], d_vals, None, ld, n_cols, P, S0, A0, None, taken, distinct,
                              k, lie_weight, trace, rows_out)


def liar_tree_device(fits, d_vals, d_active, ld, n_cols, P, S0, A, taken, distinct, k, lie_weight,
                     trace=False, rows_out=None):
    """The batch of module doc "Batches in a tree": ``_liar_picks_device`` over
    the tree fits (``fit(..., tree=True)``), ``A`` the (G, >= P) device tensor
    ``score_tree_device(above=)`` filled.  ValueError past
    ``TPE_COND_MAX_LABELS`` groups, or labels over all the groups."""
    G, D_tot = len(fits), sum(len(f.dj.models) for f in fits)
    if min(int(k), P) > 0 and (G > _L.COND_MAX_LABELS or D_tot > _L.COND_MAX_LABELS):
        raise ValueError("batch='liar-tree': %d groups of %d labels in all, at most %d of either"
                         % (G, D_tot, _L.COND_MAX_LABELS))
    return _liar_picks_device(fits, d_vals, d_active, ld, n_cols, P, S0, A, None, taken, distinct,
                              k, lie_weight, trace, rows_out)


def check_chain_lie_limits(groups, contexts):
    """ValueError where ``batch="liar-chain"`` does not reach: more than
    ``TPE_COND_MAX_LABELS`` groups, or records (every fit's context and own
    labels) over all the fits."""
    G, D_tot = len(groups), sum(len(c) + len(g) for g, c in zip(groups, contexts))
    if G > _L.COND_MAX_LABELS or D_tot > _L.COND_MAX_LABELS:
        raise ValueError("batch='liar-chain': %d groups of %d labels in all, their contexts "
                         "counted once per group, at most %d of either"
                         % (G, D_tot, _L.COND_MAX_LABELS))


def liar_chain_device(fits, d_vals, d_active, ld, n_cols, P, S0, A, B, taken, distinct, k,
                      lie_weight, trace=False, rows_out=None):
    """The batch of module doc "Batches in a chain": ``_liar_picks_device`` over
    the chain fits (``fit(..., tree="chain")``), ``A`` / ``B`` the (G, >= P)
    device tensors ``score_tree_device(above=, above_ctx=)`` filled.  ValueError
    past ``TPE_COND_MAX_LABELS`` groups, or records over all the fits, before
    anything is packed."""
    if min(int(k), P) > 0:
        check_chain_lie_limits([f.dj.models[f.n_ctx:] for f in fits],
                               [f.dj.models[:f.n_ctx] for f in fits])
    return _liar_picks_device(fits, d_vals, d_active, ld, n_cols, P, S0, A, B, taken, distinct,
                              k, lie_weight, trace, rows_out)


def refine_device(fit, d_block, ld, n_cols, k, refine, trace=None):
    """The climb of module doc "Refining" for rows [0, k) of the label-major
    device block ``d_block`` (leading dimension ``ld``, ``n_cols`` columns;
    offset-free values, as a pool's mirror holds them) under ``fit`` (the
    joint labels' fit), in place: one tpe_joint_refine, nothing read back.
    ``trace``: a dict that receives the device tensors ``J_start``, ``J_end``
    (k), ``g_end`` (k, D_c) and ``accepted`` (k, int32)."""
    eng, dj, sp = fit.eng, fit.dj, fit.sp
    t, lib = eng.torch, eng.lib
    refine = check_refine(refine)
    Dc = len(moving_labels(dj.models))
    k = int(k)
    ptrs = [None] * 4
    if trace is not None:
        trace["J_start"] = t.empty(max(k, 1), dtype=t.float64, device=eng.device)[:k]
        trace["J_end"] = t.empty(max(k, 1), dtype=t.float64, device=eng.device)[:k]
        trace["g_end"] = t.empty((max(k, 1), max(Dc, 1)), dtype=t.float64,
                                 device=eng.device)[:k, :Dc]
        trace["accepted"] = t.empty(max(k, 1), dtype=t.int32, device=eng.device)[:k]
        ptrs = [trace[name].data_ptr() for name in ("J_start", "J_end", "g_end", "accepted")]
    (below, nb, _), (above, na, _) = fit.sets
    _L.check(lib.tpe_joint_refine(dj.host.ctypes.data, dj.dev.data_ptr(), len(dj.models),
                                  None if dj.tables is None else dj.tables.data_ptr(),
                                  dj.n_tables, below.data_ptr(), nb, above.data_ptr(), na,
                                  d_block.data_ptr(), ld, n_cols, k, refine, *ptrs, sp),
             "tpe_joint_refine")


class _RefinePack(object):
    """The groups of a tree fit as tpe_joint_refine_tree takes them: the label
    records one group after the other and the group table
    (``REFINE_GROUP_DTYPE``), each on the host and on the device, the
    concatenated tables, and D_c,g per group."""
    __slots__ = ("host", "dev", "tables", "n_tables", "groups", "groups_dev", "n_cont")


def _refine_pack(fits):
    """``_RefinePack`` of ``fits`` (``fit(..., tree=True)``).  ValueError over a
    limit of the kernel."""
    eng = fits[0].eng
    t = eng.torch
    check_tree_limits([f.dj.models for f in fits])
    pk = _RefinePack()
    pk.n_cont = [len(moving_labels(f.dj.models)) for f in fits]
    rec = np.zeros(len(fits), _L.REFINE_GROUP_DTYPE)
    first = base = g_off = 0
    for g, f in enumerate(fits):
        r = rec[g]
        r["first"], r["count"], r["tab_off"] = first, len(f.dj.models), base
        r["live_col"] = -1 if g == 0 else f.dj.models[0].col
        r["n_cont"], r["g_off"] = pk.n_cont[g], g_off
        (below, nb, _), (above, na, _) = f.sets
        r["n_below"], r["n_above"] = nb, na
        r["set_below"], r["set_above"] = below.data_ptr(), above.data_ptr()
        first, base, g_off = first + len(f.dj.models), base + f.dj.n_tables, g_off + pk.n_cont[g]
    pk.host = np.concatenate([f.dj.host for f in fits])
    pk.dev = t.from_numpy(pk.host.view(np.uint8).copy()).to(eng.device)
    tabs = [f.dj.tables for f in fits if f.dj.tables is not None]
    pk.tables, pk.n_tables = (t.cat(tabs) if tabs else None), base
    pk.groups = rec
    pk.groups_dev = t.from_numpy(rec.view(np.uint8).copy()).to(eng.device)
    return pk


def refine_tree_device(fits, d_block, d_active, ld, n_cols, k, refine, trace=None):
    """The climb of module doc "Refining in a tree" for rows [0, k) of the
    label-major device block ``d_block`` / ``d_active`` (bytes; leading
    dimension ``ld``, ``n_cols`` columns; offset-free values) under ``fits``
    (``fit(..., tree=True)``), in place: one tpe_joint_refine_tree, nothing read
    back.  ``trace``: a dict that receives the device tensors ``J_start``,
    ``J_end`` (k, G), ``g_end`` (k, sum of D_c,g) and ``accepted`` (k, G; int32).
    ValueError past ``TPE_REFINE_MAX_CONT`` continuous labels in a group, or
    ``TPE_COND_MAX_LABELS`` groups, or labels over all the groups."""
    eng, sp = fits[0].eng, fits[0].sp
    t, lib = eng.torch, eng.lib
    refine = check_refine(refine)
    pk = _refine_pack(fits)
    k, G, Dc = int(k), len(fits), sum(pk.n_cont)
    ptrs = [None] * 4
    if trace is not None:
        for name, cols, dtype in (("J_start", G, t.float64), ("J_end", G, t.float64),
                                  ("g_end", Dc, t.float64), ("accepted", G, t.int32)):
            trace[name] = t.empty((max(k, 1), max(cols, 1)), dtype=dtype,
                                  device=eng.device)[:k, :cols]
        # (g_end's rows are sum D_c,g long in the call: a narrower view would not be)
        if Dc == 0:
            trace["g_end"] = t.empty((k, 0), dtype=t.float64, device=eng.device)
        ptrs = [trace[name].data_ptr() for name in ("J_start", "J_end", "g_end", "accepted")]
    _L.check(lib.tpe_joint_refine_tree(
        pk.host.ctypes.data, pk.dev.data_ptr(), len(pk.host),
        None if pk.tables is None else pk.tables.data_ptr(), pk.n_tables, pk.groups.ctypes.data,
        pk.groups_dev.data_ptr(), G, d_block.data_ptr(), d_active.data_ptr(), ld, n_cols, k,
        refine, *ptrs, sp), "tpe_joint_refine_tree")


def loo_device(eng, domain, hist, seen, gamma, n_cols, grid=None, prior_weight=1.0,
               linear_forgetting=25, cat_smoothing=CAT_SMOOTHING, tree=False):
    """``loo_numpy`` on the device: Q_set of every group's below and above set
    over ``grid`` as a numpy (G, 2, B) array.  One tpe_joint_loo per set with n
    >= 2 -- every pair of its rows once, for all B multipliers -- reading the
    history ``seen`` (``fit``'s tuple) through the set's row list; one readback
    after the last."""
    t, lib = eng.torch, eng.lib
    grid = np.ascontiguousarray(check_grid(grid))
    sets = loo_sets(domain, hist, gamma, tree)
    _alive, sv, sa, sld, srows, _n = seen
    view = hist.rows if srows is not None else None  # (positions -> rows of the mirror)
    out = t.zeros((len(sets), 2, grid.size), dtype=t.float64, device=eng.device)
    sp = stream_ptr(eng)
    keep = []  # (what a launch reads stays allocated until the readback)
    for g, (models, pair) in enumerate(sets):
        if max(rows.size for rows in pair) < 2:
            continue
        dj = _device_labels(eng, models, cat_smoothing)
        n_quant = sum(m.kind == _L.JOINT_QUANT for m in models)
        for which, rows in enumerate(pair):
            n = int(rows.size)
            if n < 2:  # (Q_set = 0: ``out`` holds it)
                continue
            if view is not None:
                rows = np.asarray(view)[rows]
            v = forgetting_weights(n, linear_forgetting)
            drows = t.from_numpy(np.ascontiguousarray(rows, np.int32)).to(eng.device)
            dv = t.from_numpy(np.ascontiguousarray(v)).to(eng.device)
            scratch = t.empty(lib.tpe_joint_loo_scratch_bytes(len(models), n_quant, n, grid.size),
                              dtype=t.uint8, device=eng.device)
            keep.append((dj, drows, dv, scratch))
            _L.check(lib.tpe_joint_loo(
                dj.host.ctypes.data, dj.dev.data_ptr(), len(models),
                None if dj.tables is None else dj.tables.data_ptr(), dj.n_tables, sv, sa, sld,
                n_cols, drows.data_ptr(), n, dv.data_ptr(), float(v.sum()), float(prior_weight),
                grid.ctypes.data, grid.size, out[g, which].data_ptr(), scratch.data_ptr(), sp),
                "tpe_joint_loo")
    return out.cpu().numpy()


def loo_label_curves(eng, domain, hist, seen, gamma, n_cols, grid=None, prior_weight=1.0,
                     linear_forgetting=25, cat_smoothing=CAT_SMOOTHING, tree=False):
    """``loo_label_numpy`` on the device, as the function ``curve(mult, label)``
    -> (2, B) numpy: two tpe_joint_loo_label calls (the label's group's below
    and above set; a set with n < 2 is 0 without a launch) and one readback.
    A group's label records, row lists, weights and scratch go up at the first
    call for one of its labels and serve every later one."""
    t, lib = eng.torch, eng.lib
    grid = np.ascontiguousarray(check_grid(grid))
    sets = loo_sets(domain, hist, gamma, tree)
    _alive, sv, sa, sld, srows, _n = seen
    view = hist.rows if srows is not None else None  # (positions -> rows of the mirror)
    sp = stream_ptr(eng)
    out = t.zeros((2, grid.size), dtype=t.float64, device=eng.device)
    where = {lab: (g, d) for g, d, lab in banded_labels(sets)}
    groups = {}

    def group(g):
        """Group g on the device: (label records, per set None or (rows, v, sum v,
        scratch, n))."""
        if g not in groups:
            models, pair = sets[g]
            dj = _device_labels(eng, models, cat_smoothing)
            n_quant = sum(m.kind == _L.JOINT_QUANT for m in models)
            up = []
            for rows in pair:
                n = int(rows.size)
                if n < 2:
                    up.append(None)
                    continue
                if view is not None:
                    rows = np.asarray(view)[rows]
                v = forgetting_weights(n, linear_forgetting)
                need = lib.tpe_joint_loo_label_scratch_bytes(len(models), n_quant, n, grid.size)
                up.append((t.from_numpy(np.ascontiguousarray(rows, np.int32)).to(eng.device),
                           t.from_numpy(np.ascontiguousarray(v)).to(eng.device), float(v.sum()),
                           t.empty(need, dtype=t.uint8, device=eng.device), n))
            groups[g] = (dj, up)
        return groups[g]

    def curve(mult, label):
        if label not in where:
            raise ValueError("%r is not a label with a bandwidth of the joint criterion"
                             % (label,))
        g, d = where[label]
        dj, up = group(g)
        h = np.asarray([mult.get(m.label, BANDWIDTH) for m in dj.models], np.float64)
        out.zero_()
        for which, one in enumerate(up):
            if one is None:  # (Q_set = 0: ``out`` holds it)
                continue
            drows, dv, sum_v, scratch, n = one
            _L.check(lib.tpe_joint_loo_label(
                dj.host.ctypes.data, dj.dev.data_ptr(), len(dj.models),
                None if dj.tables is None else dj.tables.data_ptr(), dj.n_tables, sv, sa, sld,
                n_cols, drows.data_ptr(), n, dv.data_ptr(), sum_v, float(prior_weight),
                h.ctypes.data, d, grid.ctypes.data, grid.size, out[which].data_ptr(),
                scratch.data_ptr(), sp), "tpe_joint_loo_label")
        return out.cpu().numpy()  # (the scratch is free for the next call after it)

    return curve


def loo_label_device(eng, domain, hist, seen, gamma, n_cols, grid=None, prior_weight=1.0,
                     linear_forgetting=25, cat_smoothing=CAT_SMOOTHING, tree=False, sweeps=2):
    """``loo_label_fit_numpy`` on the device: (mapping, visited).  The start is
    ``loo_device``'s scalar choice; then per visited label the (2, B) curves of
    ``loo_label_curves`` -- the choice is made on the host and steers the next
    call."""
    grid, sweeps = check_grid(grid), check_sweeps(sweeps)
    sets = loo_sets(domain, hist, gamma, tree)
    args = (eng, domain, hist, seen, gamma, n_cols, grid, prior_weight, linear_forgetting,
            cat_smoothing, tree)
    sizes = [[rows.size for rows in pair] for _m, pair in sets]
    return loo_label_choice(grid, loo_device(*args), sizes,
                            [lab for _g, _d, lab in banded_labels(sets)],
                            loo_label_curves(*args), sweeps)


# -- groups on the device (module doc, "Groups") ---------------------------------
def sample_tree_device(fits, seed, d_vals, ld, n_cols, row_base, n_rows):
    """``sample_device`` per fit of ``fits`` (``fit(..., tree=True)``): every
    group's columns for all the rows, the root group under
    ``component_key(seed)``, the others under their ``group_component_key``."""
    for g, f in enumerate(fits):
        key = None if g == 0 else group_component_key(seed, f.group[0])
        sample_device(f, seed, d_vals, ld, n_cols, row_base, n_rows, comp_key=key)


def score_tree_device(fits, d_vals, d_active, ld, n_cols, P, out, parts=None, above=None,
                      above_ctx=None):
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
    compacted on the group's first own label, not the context's.

    ``above`` (``tree=True`` fits): a (G, >= P) device tensor that receives A_g
    = log L_above,g at the rows in which group g is live (module doc, "Batches
    in a tree"); its other places are not written.  Row 0 is the root's
    subtrahend itself; a group's dense temporary goes to its rows by one
    tpe_rows_scatter per window.  None: exactly the calls above.

    ``above_ctx`` (``tree="chain"`` fits, beside ``above``): a (G, >= P) device
    tensor; a fit with a context leaves A_g = log L_above in ``above[g]`` and B_g =
    log L_ctx,above in ``above_ctx[g]`` at its live rows (module doc, "Batches in
    a chain") from the merge that forms them, tpe_joint_chain_rows_keep in
    tpe_joint_chain_rows' place and no scatter; a fit without one fills
    ``above[g]`` as above.  Both None: exactly the calls above."""
    eng = fits[0].eng
    t, lib = eng.torch, eng.lib
    score_device(fits[0], d_vals, ld, n_cols, P, out, keep_above=None if above is None else above[0])
    if parts is not None:
        parts[0, :P].copy_(out[:P])
    if len(fits) == 1 or P == 0:
        return
    rows = t.empty(P, dtype=t.int64, device=eng.device)
    count = t.empty(1, dtype=t.int64, device=eng.device)
    cscratch = t.empty(lib.tpe_rows_compact_scratch_bytes(P), dtype=t.uint8, device=eng.device)
    for g, f in enumerate(fits[1:], 1):
        flags = d_active.data_ptr() + f.dj.models[f.n_ctx].col * ld
        _L.check(lib.tpe_rows_compact(flags, P, rows.data_ptr(), count.data_ptr(),
                                      cscratch.data_ptr(), f.sp), "tpe_rows_compact")
        _score_fit(f, d_vals, ld, n_cols, P, out, listed=(rows, count),
                   above_to=None if above is None else above[g],
                   ctx_to=None if above_ctx is None else above_ctx[g],
                   j_to=None if parts is None else parts[g])


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
