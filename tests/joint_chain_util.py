"""The chain-rule criterion (``joint="chain"``) restated with scalar loops, for
the tests.

Written from the model's definition (hyperopt_amd/joint.py's module text,
"Chains") and independent of ``hyperopt_amd/joint.py``: groups
and contexts are read off ``domain.live_program()`` here, a set is built by
``tests/joint_util.py``'s ``set_components`` over ``ctx + g`` (which takes D
and the dropped rows from the list it is given), the full mixture is its
``log_l`` and the marginal is ``log_l`` over the first n_ctx labels of the very
same components.  Only the history and its split come from the package.

The cases the CPU and the GPU tests share are at the end.
"""
import numpy as np

from hyperopt_amd import Domain, hp, tpe
from tests import joint_tree_util as TU
from tests import joint_util as U


def contexts_of(domain):
    """[ctx labels] per group of ``joint_tree_util.groups_of``: the labels
    outside the group that are live whenever it is, without the selectors all
    its clauses hold at one branch."""
    prog = domain.live_program()
    out = []
    for clauses, labs in TU.groups_of(domain):
        ctx = []
        for lab in domain.params:
            if lab in labs or clauses == ((),):
                continue
            whenever = True
            for c in clauses:
                if not any(all(pair in c for pair in lc) for lc in prog[lab]):
                    whenever = False
            branches = [[b for s, b in c if s == lab] for c in clauses]
            fixed = all(len(b) == 1 for b in branches) and len({b[0] for b in branches}) == 1
            if whenever and not fixed:
                ctx.append(lab)
        out.append(ctx)
    return out


def chain_reference(domain, trials, vals, active, prior_weight=1.0, gamma=0.25, lf=25,
                    bandwidth=0.2, cat_smoothing=1.0):
    """(S, C, log L_below, log L_above, log L_ctx,below, log L_ctx,above,
    [(n_below, n_above)]) of the rows ``vals`` ((P, L) stored values) with
    activity ``active``: S (P,), the matrices (P, G), NaN where the group is
    not live in the row; the marginals NaN for a group with an empty context."""
    labels = list(domain.params)
    groups = TU.groups_of(domain)
    contexts = contexts_of(domain)
    hist = tpe.collect_history(trials, labels)
    isb, isa = tpe.split_masks(hist, gamma) if hist.tids.size else ([], [])
    P, G = vals.shape[0], len(groups)
    Cm, LB, LA, CB, CA = (np.full((P, G), np.nan) for _ in range(5))
    ns = []
    a = float(cat_smoothing)
    for g, ((_clauses, labs), ctx) in enumerate(zip(groups, contexts)):
        names = ctx + labs
        n_ctx = len(ctx)
        cols = [labels.index(lab) for lab in names]
        infos = [U.label_info(domain.specs[lab]) for lab in names]
        sets = [U.set_components(infos, cols, hist, mask, lf, prior_weight, bandwidth)
                for mask in (isb, isa)]
        ns.append((sets[0][2], sets[1][2]))
        for r in range(P):
            if not all(active[r, labels.index(lab)] for lab in labs):
                continue
            x = [float(vals[r, j]) for j in cols]
            LB[r, g], LA[r, g] = (U.log_l(infos, logw, comps, x, a) for logw, comps, _n in sets)
            with np.errstate(invalid="ignore"):
                if n_ctx:
                    CB[r, g], CA[r, g] = (U.log_l(infos[:n_ctx], logw, comps[:n_ctx], x[:n_ctx], a)
                                          for logw, comps, _n in sets)
                    Cm[r, g] = (LB[r, g] - CB[r, g]) - (LA[r, g] - CA[r, g])
                else:
                    Cm[r, g] = LB[r, g] - LA[r, g]
    S = TU.fold_live(Cm, TU.group_live(domain, np.asarray(active, bool)))
    return S, Cm, LB, LA, CB, CA, ns


def tolerance(LB, LA, CB, CA):
    """Per row, 1e-6 * the sum over the live groups of |log L_below| + |log
    L_above| plus, for a group with a context, the two marginals' |.| (the
    project's fp64 log-density rule, as ``joint_tree_util.tolerance``)."""
    return 1e-6 * sum(np.nansum(np.abs(m), 1) for m in (LB, LA, CB, CA))


def column_tolerance(ref, g):
    """The same rule for column g of C alone (NaN where g is not live)."""
    return 1e-6 * sum(np.nan_to_num(np.abs(m[:, g]), nan=0.0, posinf=np.inf)
                      for m in ref[2:6])


# -- the cases -------------------------------------------------------------------
def cross_space():
    """A root label ``a`` that interacts with ``b`` inside branch 0 of ``v``."""
    return {"a": hp.choice("a", [0, 1, 2, 3]),
            "v": hp.choice("v", [{"b": hp.choice("b", [0, 1, 2, 3])},
                                 {"c": hp.uniform("c", 0, 1)}])}


def cross_level_case():
    """(domain, trials): 64 trials of branch 0 -- every (a, b) cell four times
    in ``joint_util.diagonal_case``'s order, loss [a != b] + 1e-6 tid -- then
    36 of branch 1 under ``RandomState(5)``, per trial ``a = rng.randint(4)``
    then ``c = rng.uniform()``, loss 2 + 1e-6 tid.  With
    ``gamma=joint_tree_util.GAMMA_DIAGONAL`` the below side is the 16
    diagonal trials."""
    _space, configs, _losses = U.diagonal_case(hp)
    domain = Domain(lambda x: 0, cross_space())
    rng = np.random.RandomState(5)
    cfgs = [dict(c, v=0) for c in configs]
    for _ in range(36):
        a = int(rng.randint(4))
        cfgs.append({"v": 1, "a": a, "c": float(rng.uniform())})
    losses = [float(c["a"] != c["b"]) + 1e-6 * tid if c["v"] == 0 else 2.0 + 1e-6 * tid
              for tid, c in enumerate(cfgs)]
    return domain, U.make_trials(domain, cfgs, losses)


def cross_pool_rows():
    """The 16 (a, b) configurations of branch 0 in row order 4 a + b, then one
    row of branch 1."""
    return [dict(r, v=0) for r in U.diagonal_pool_rows()] + [{"v": 1, "a": 1, "c": 0.5}]


DIAGONAL = [0, 5, 10, 15]


def rooted_branch_space():
    """``joint_tree_util.branch_space`` with a root label added: the context of
    both of its groups."""
    return dict(TU.branch_space(), r=hp.uniform("r", -1, 1))


def rooted_edge_histories():
    """``joint_tree_util.edge_histories`` with ``r`` in every trial, and one
    more: a foreign trial that has (a, b) but lacks the context label ``r`` --
    it is dropped from that group's sets and n shrinks."""
    rng = np.random.RandomState(3)
    out = {}
    for name, (configs, losses) in TU.edge_histories().items():
        out[name] = ([dict(c, r=float(rng.uniform(-1, 1))) for c in configs], list(losses))
    configs, losses = out["above_only"]
    out["foreign_context"] = (configs + [{"v": 0, "a": 1, "b": 1}], losses + [9.0])
    return out


def rooted_pool_rows():
    rng = np.random.RandomState(4)
    return [dict(row, r=float(rng.uniform(-1, 1))) for row in TU.branch_pool_rows()]
