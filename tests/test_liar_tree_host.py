"""``joint.liar_tree_numpy`` (joint.py, "Batches in a tree") against the scalar
restatement below -- one loop per index on tests/joint_util.py's factors and
tests/joint_tree_util.py's groups -- and ``batch="liar-tree"``'s argument errors.
Tolerance: as test_liar_host.py, 1e-9 of |S_0| plus per live group |U_0| + |U_k|.
"""
import math

import numpy as np
import pytest

from hyperopt_amd import Domain, hp, rand, tpe
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from oracle import tpe_oracle as O
from tests import joint_tree_util as TU
from tests import joint_util as U
from tests import liar_util as LU

KW = dict(prior_weight=0.7, gamma=0.3, bandwidth=0.25, cat_smoothing=0.5)


def group_sets(domain, trials, gamma=0.25, lf=25, prior_weight=1.0, bandwidth=0.2):
    """Per group (infos, cols, sigma, log W) of its lie under the above set."""
    labels = list(domain.params)
    hist = tpe.collect_history(trials, labels)
    isa = tpe.split_masks(hist, gamma)[1] if hist.tids.size else []
    out = []
    for _clauses, labs in TU.groups_of(domain):
        cols = [labels.index(lab) for lab in labs]
        infos = [U.label_info(domain.specs[lab]) for lab in labs]
        n = sum(1 for r in range(hist.tids.size) if isa[r] and all(hist.active[r, j] for j in cols))
        sigma = [bandwidth * i["sigma"] * float(max(n, 1)) ** (-1.0 / (len(cols) + 4)) for i in infos]
        total = sum(float(w) for w in O.linear_forgetting_weights(n, lf)) + float(prior_weight)
        out.append((infos, cols, sigma, math.log(total)))
    return out


def tree_lie_picks(sets, vals, live, S0, A, log_lie, a, k, gone=None):
    """The definition, loop by loop; ``live`` / ``A``: (P, G).  Returns rows,
    S_at_pick, S_k, U_0 and U_k ((P, G), NaN where dead), and per pick the gap to
    the best other free row over 1e-6 sum_g (|U_g0| + |U_g|) of the two rows."""
    P, G = vals.shape[0], len(sets)
    gone = [False] * P if gone is None else [bool(g) for g in gone]
    U0 = [[sets[g][3] + float(A[r, g]) if live[r, g] else float("nan") for g in range(G)]
          for r in range(P)]
    Uc, S = [list(u) for u in U0], [float(s) for s in S0]
    rows, at, margin = [], [], []

    def bound(r):
        return 1e-6 * sum(abs(U0[r][g]) + abs(Uc[r][g]) for g in range(G)
                          if live[r, g] and math.isfinite(U0[r][g]))

    for _ in range(min(max(int(k), 0), P)):
        p = LU.first_row(S, gone)
        if p < 0:
            break
        q = max((r for r in range(P) if r != p and not gone[r]), key=lambda r: S[r], default=p)
        margin.append(float("nan") if S[p] != S[p] else float("inf") if q == p else
                      (S[p] - S[q]) / max(bound(p), bound(q), 1e-300))
        rows.append(p)
        at.append(S[p])
        gone[p] = True
        comps = {g: LU.lie_component(infos, [[float(vals[p, j]) for j in cols]], 0, sigma)
                 for g, (infos, cols, sigma, _w) in enumerate(sets) if live[p, g]}
        for r in range(P):
            s = float(S0[r])
            for g, (infos, cols, _sigma, _w) in enumerate(sets):
                if not live[r, g]:
                    continue
                if g in comps:
                    c = log_lie
                    for d, info in enumerate(infos):
                        c = c + U.factor(info, float(vals[r, cols[d]]), comps[g][d], a)
                    if c != U.NEG_INF:
                        m = max(c, Uc[r][g])
                        Uc[r][g] = U.NEG_INF if m == U.NEG_INF else \
                            m + math.log(math.exp(Uc[r][g] - m) + math.exp(c - m))
                if math.isfinite(U0[r][g]):
                    s = s - (Uc[r][g] - U0[r][g])
            S[r] = s
    return dict(rows=rows, S_at_pick=np.asarray(at), S_k=np.asarray(S), U_0=np.asarray(U0),
                U_k=np.asarray(Uc), margin=np.asarray(margin))


def tolerance(ref, rel):
    """``rel`` times the sum over the row's live groups of |U_0| + |U_k|."""
    fin = np.isfinite(ref["U_0"])
    return rel * np.where(fin, np.abs(ref["U_0"]) + np.abs(ref["U_k"]), 0.0).sum(1)


def _branch_case():
    domain, trials = TU.branch_diagonal_case()
    rng = np.random.RandomState(3)
    pool = tpe.Pool(domain, [rand.sample_config(domain, rng) for _ in range(60)])
    hist = tpe.collect_history(trials, pool.labels)
    S0, _J, _below, A = J.score_numpy(domain, hist, pool.vals, pool.active, return_parts=True,
                                      tree=True, **KW)
    return domain, trials, hist, pool.vals, pool.active.astype(bool), S0, A


def test_liar_tree_numpy_matches_scalar_restatement():
    domain, trials, hist, vals, active, S0, A = _branch_case()
    live = TU.group_live(domain, active)
    assert live[:, 1].any() and live[:, 2].any() and len(TU.groups_of(domain)) == 3
    ref = tree_lie_picks(group_sets(domain, trials, KW["gamma"], 25, KW["prior_weight"],
                                    KW["bandwidth"]), vals, live, S0, A, math.log(1.3),
                         KW["cat_smoothing"], 6)
    kw = dict(KW, active=active, lie_weight=1.3)
    rows, at, S_k = J.liar_tree_numpy(domain, hist, vals, 6, S0=S0, A=A, **kw)
    assert rows.tolist() == ref["rows"] and len(set(ref["rows"])) == 6
    bound = tolerance(ref, 1e-9) + 1e-9 * np.abs(S0)
    assert (np.abs(S_k - ref["S_k"]) <= bound).all()
    assert (np.abs(at - ref["S_at_pick"]) <= bound[rows]).all()
    assert (S_k <= S0).all() and (S_k[rows] < S0[rows]).all()
    rows1, at1, _S = J.liar_tree_numpy(domain, hist, vals, 1, S0=S0, A=A, **kw)  # k = 1
    assert rows1.tolist() == [int(np.argmax(S0))] and at1[0] == S0[rows1[0]]
    again = J.liar_tree_numpy(domain, hist, vals, 6, **kw)  # (from the history alone)
    assert again[0].tolist() == ref["rows"] and (again[2] == S_k).all()


def test_flat_space_has_the_bits_of_liar_numpy():
    domain = Domain(lambda x: 0, U.all_kinds_space(hp))
    rng = np.random.RandomState(5)
    trials = U.make_trials(domain, [rand.sample_config(domain, rng) for _ in range(40)],
                           rng.uniform(size=40))
    pool = tpe.Pool(domain, [rand.sample_config(domain, rng) for _ in range(30)])
    hist = tpe.collect_history(trials, pool.labels)
    kw = dict(KW, taken=(rng.uniform(size=30) < 0.3).astype(np.uint8), lie_weight=0.8)
    flat = J.liar_numpy(domain, hist, pool.vals, 5, **kw)
    tree = J.liar_tree_numpy(domain, hist, pool.vals, 5, **kw)
    assert flat[0].tolist() == tree[0].tolist() and len(flat[0]) == 5
    for a, b in zip(flat[1:], tree[1:]):
        assert (a.view(np.uint64) == b.view(np.uint64)).all()


def test_a_branch_live_in_the_pick_alone_moves_the_root_only():
    """The pick is branch 1's only row: the others are penalised through the root alone."""
    domain, _trials, hist, vals, active, S0, A = _branch_case()
    v = vals[:, list(domain.params).index("v")]
    keep = np.concatenate([np.flatnonzero(v == 1)[:1], np.flatnonzero(v == 0)])
    vals, active, S0, A = vals[keep], active[keep], S0[keep], A[keep]
    S0[0] = S0.max() + 1.0  # the lone row leads
    rows, _at, S_1 = J.liar_tree_numpy(domain, hist, vals, 1, active, S0=S0, A=A, **KW)
    root = J.liar_numpy(domain, hist, vals, 1, S0=S0, A0=A[:, 0], **KW)[2]
    assert rows.tolist() == [0] and (S_1[1:].view(np.uint64) == root[1:].view(np.uint64)).all()
    assert S_1[0] < root[0] < S0[0]  # the pick itself: the root's penalty and its group's


def test_argument_errors():
    domain, trials, hist, vals, active, _S0, _A = _branch_case()
    pool = tpe.Pool.from_arrays(domain, vals[:3], active[:3])
    grid = tpe.GridPool(domain, {"v": [0], "a": [0, 1], "b": [0, 1], "c": [0.5]}, joint="tree")
    ids = [100, 101]
    for kw, text in ((dict(joint=True), "batch='liar'"), (dict(), "joint='tree'"),
                     (dict(joint="chain"), "ratio"), (dict(joint="tree", pool=grid), "GridPool"),
                     (dict(joint="tree", lie_weight=0.0), "finite number > 0")):
        with pytest.raises(ValueError, match=text):
            tpe.suggest_from_pool(ids, domain, trials, 0, batch="liar-tree",
                                  **dict(dict(pool=pool), **kw))
        if "pool" not in kw:
            with pytest.raises(ValueError, match=text):
                tpe.suggest_sampled(ids, domain, trials, 0, batch="liar-tree", **kw)
    for kw, text in ((dict(pool=grid, joint="tree"), "GridPool"),
                     (dict(pool=pool, joint="chain"), "joint='chain' keeps no")):
        with pytest.raises(ValueError, match=text):
            tpe.pick_batch(domain, trials, kw["pool"], 2, joint=kw["joint"])
    with pytest.raises(ValueError, match="lie_weight"):
        J.liar_tree_numpy(domain, hist, vals, 2, lie_weight=0.0)


@pytest.mark.parametrize("batch,joint", [(None, "tree"), ("liar", True), ("liar-tree", "tree")])
def test_the_calls_each_batch_builds(monkeypatch, batch, joint):
    """``None`` and ``"liar"`` reach the scoring and the pick as they always did."""
    domain, trials, _hist, vals, active, _S0, _A = _branch_case()
    pool = tpe.Pool.from_arrays(domain, vals[:8], active[:8])
    calls = []
    monkeypatch.setattr(pool_mod, "_score_device", lambda *a, **kw: calls.append(
        ("score", a[3], a[4:], set(kw))) or ("eng", "mirror"))
    for name in ("_topk_device", "_liar_device"):
        monkeypatch.setattr(pool_mod, name, lambda *a, name=name: calls.append(
            (name, a)) or np.asarray([6, 2]))
    tpe.suggest_from_pool([100, 101], domain, trials, 0, pool=pool, joint=joint, batch=batch,
                          lie_weight=2.0, verbose=False)
    (_s, st, rest, kws), (which, args) = calls
    assert rest == (False,) and kws == {"hist"}
    assert st.joint == dict(bandwidth=J.BANDWIDTH, cat_smoothing=J.CAT_SMOOTHING,
                            tree=joint == "tree")
    assert (st.lie, st.lie_tree) == (None if batch is None else 2.0, batch == "liar-tree")
    if batch is None:
        assert (which, args) == ("_topk_device", ("eng", "mirror", 8, 2, None))
    else:
        assert (which, args) == ("_liar_device", ("eng", "mirror", 8, 2, None, 2.0, False,
                                                  batch == "liar-tree"))
