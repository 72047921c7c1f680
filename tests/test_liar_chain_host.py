"""``joint.liar_chain_numpy`` (joint.py, "Batches in a chain") against the scalar
restatement below (liar_util's lie component over ``chain_reference``'s fits), its bits,
errors and settings.  Tolerance: 1e-9 of |S_0| plus per live fit |U_0| + |U_k| + |V_0| + |V_k|.
"""
import math

import numpy as np
import pytest

from hyperopt_amd import hp, rand, tpe
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from oracle import tpe_oracle as O
from tests import joint_chain_util as CU
from tests import joint_tree_util as TU
from tests import joint_util as U
from tests import liar_util as LU
from tests.liar_chain_util import chain_case

KW = dict(prior_weight=0.7, gamma=0.3, bandwidth=0.25, cat_smoothing=0.5)


def chain_lie_picks(sets, vals, live, S0, A, B, log_lie, a, k):
    """The definition, loop by loop; ``live`` / ``A`` / ``B``: (P, G); ``sets``: per
    chain fit (infos, cols, n_ctx, sigma, log W).  Returns the rows and S_k."""
    def join(u, c):
        m = max(u, c)
        return u if c == U.NEG_INF else m + math.log(math.exp(u - m) + math.exp(c - m))

    P, log_w, ctx = vals.shape[0], np.asarray([s[4] for s in sets]), [s[2] > 0 for s in sets]
    U0, V0 = np.where(live, log_w + A, 0.0), np.where(live & ctx, log_w + B, 0.0)
    Uc, Vc, S, gone, rows = U0.copy(), V0.copy(), list(S0), [False] * P, []
    for _ in range(k):
        rows.append(LU.first_row(S, gone))
        p = rows[-1]
        gone[p] = True
        comps = {g: LU.lie_component(infos, [[float(vals[p, j]) for j in cols]], 0, sigma)
                 for g, (infos, cols, _n, sigma, _w) in enumerate(sets) if live[p, g]}
        for r in range(P):
            S[r] = float(S0[r])
            for g, (infos, cols, n_ctx, _sigma, _w) in enumerate(sets):
                if live[r, g] and g in comps:
                    c = log_lie
                    for d, info in enumerate(infos):
                        if n_ctx and d == n_ctx:
                            Vc[r, g] = join(Vc[r, g], c)
                        c = c + U.factor(info, float(vals[r, cols[d]]), comps[g][d], a)
                    Uc[r, g] = join(Uc[r, g], c)
                if live[r, g]:
                    S[r] = S[r] - ((Uc[r, g] - U0[r, g]) - (Vc[r, g] - V0[r, g]))
    return rows, np.asarray(S)


def test_liar_chain_numpy_matches_scalar_restatement():
    domain, trials, pool = chain_case(50, 1)
    vals, active = pool.vals, pool.active.astype(bool)
    ctxs, live = CU.contexts_of(domain), TU.group_live(domain, active)
    assert len(ctxs[0]) == 0 and len(TU.groups_of(domain)[0][1]) == 3 and len(ctxs) == 7
    assert any("s" in c for c in ctxs) and any("w" in c for c in ctxs) and live[:, 1:6].any(0).all()
    S0, _C, _LB, A, _CB, B, ns = CU.chain_reference(domain, trials, vals, active, **KW)
    sets = []
    for (_clauses, labs), ctx, (_nb, n) in zip(TU.groups_of(domain), ctxs, ns):
        infos = [U.label_info(domain.specs[lab]) for lab in ctx + labs]
        sigma = [KW["bandwidth"] * i["sigma"] * float(max(n, 1)) ** (-1.0 / (len(infos) + 4))
                 for i in infos]
        total = sum(map(float, O.linear_forgetting_weights(n, 25))) + KW["prior_weight"]
        sets.append((infos, [pool.labels.index(lab) for lab in ctx + labs], len(ctx), sigma,
                     math.log(total)))
    rows_ref, S_ref = chain_lie_picks(sets, vals, live, S0, A, B, math.log(1.3),
                                      KW["cat_smoothing"], 6)
    kw = dict(KW, active=active, lie_weight=1.3, S0=S0, A=A, B=B)
    hist = tpe.collect_history(trials, pool.labels)
    rows, at, S_k, *state = J.liar_chain_numpy(domain, hist, vals, 6, return_state=True, **kw)
    assert rows.tolist() == rows_ref and len(set(rows_ref)) == 6
    assert (np.abs(S_k - S_ref) <= 1e-9 * (np.nansum(np.abs(state), (0, 2)) + np.abs(S0))).all()
    rows1, at1, _S = J.liar_chain_numpy(domain, hist, vals, 1, **kw)  # k = 1
    assert rows1.tolist() == [int(np.argmax(S0))] and at1[0] == S0[rows1[0]] == at[0]


@pytest.mark.parametrize("shape", ["branch", "flat"])
def test_empty_contexts_have_the_bits_of_the_tree_and_the_flat_batch(shape):
    rng = np.random.RandomState(5)
    if shape == "branch":  # the root is the selector alone: every context is empty
        domain, trials = TU.branch_diagonal_case()
        other = J.liar_tree_numpy
    else:
        domain, trials, _pool = chain_case(1, 5, lambda: U.all_kinds_space(hp))
        other = J.liar_numpy
    pool = tpe.Pool(domain, [rand.sample_config(domain, rng) for _ in range(30)])
    hist = tpe.collect_history(trials, pool.labels)
    kw = dict(KW, taken=(rng.uniform(size=30) < 0.3).astype(np.uint8), lie_weight=0.8)
    want, got = other(domain, hist, pool.vals, 5, **kw), J.liar_chain_numpy(domain, hist, pool.vals,
                                                                           5, **kw)
    assert want[0].tolist() == got[0].tolist() and len(got[0]) == 5
    for a, b in zip(want[1:], got[1:]):
        assert (a.view(np.uint64) == b.view(np.uint64)).all()


def test_a_row_far_inside_the_group_at_the_picks_context_gains():
    """Pick (a, b) of branch 0: the row (a, b + 2) shares the context ``a`` and
    misses ``b``, so the marginal at ``a`` rises by more than the joint there."""
    domain, trials = CU.cross_level_case()
    pool = tpe.Pool(domain, CU.cross_pool_rows())
    rows, _at, _S, U0, U1, V0, V1 = J.liar_chain_numpy(
        domain, tpe.collect_history(trials, pool.labels), pool.vals, 1, pool.active,
        gamma=TU.GAMMA_DIAGONAL, return_state=True)
    p, g = int(rows[0]), CU.contexts_of(domain).index(["a"])  # (the first such fit: ``b``'s)
    pen = (U1 - U0)[:, g] - (V1 - V0)[:, g]
    far = 4 * (p // 4) + (p % 4 + 2) % 4
    assert p in CU.DIAGONAL and pen[far] < 0.0 < pen[p] and (V1 - V0)[far, g] > 0.0


@pytest.mark.parametrize("call,kw,text", [(c, kw, text) for calls, kw, text in [
    ("fs", dict(joint=True), "joint='chain'"), ("fs", dict(joint="tree"), "joint='chain'"),
    ("fs", dict(), "joint='chain'"), ("f", dict(joint="chain", grid=True), "GridPool"),
    ("fs", dict(joint="chain", lie_weight=0.0), "finite number > 0"),
    ("s", dict(joint="chain", refine=2), "refine"),
    ("f", dict(joint="chain", batch="liars"), "'liar-tree' .joint='tree'. or 'liar-chain'"),
    ("s", dict(joint="chain", refine_tree=2), "refine"), ("p", dict(joint="tree"), "joint='chain'"),
    ("p", dict(joint="chain", batch=None), "joint='chain' keeps no"),  # (no batch: as before)
    ("n", dict(lie_weight=0.0), "lie_weight"),
    ("l", dict(G=129, n_ctx=0), "at most 128"), ("l", dict(G=33, n_ctx=3), "at most 128")]
    for c in calls])
def test_argument_errors(call, kw, text):
    domain, trials = TU.branch_diagonal_case()
    pool = tpe.Pool(domain, TU.branch_pool_rows()[:3])
    kw = dict(dict(batch="liar-chain"), **kw)
    if kw.pop("grid", False):
        pool = tpe.GridPool(domain, {"v": [0], "a": [0, 1], "b": [0, 1], "c": [0.5]}, joint="tree")
    with pytest.raises(ValueError, match=text):
        if call == "f":
            tpe.suggest_from_pool([100, 101], domain, trials, 0, pool=pool, **kw)
        elif call == "s":
            tpe.suggest_sampled([100, 101], domain, trials, 0, **kw)
        elif call == "p":
            tpe.pick_batch(domain, trials, pool, 2, **kw)
        elif call == "n":
            J.liar_chain_numpy(domain, tpe.collect_history(trials, pool.labels), pool.vals, 2,
                               lie_weight=kw["lie_weight"])
        else:
            J.check_chain_lie_limits([["x"]] * kw["G"], [["a"] * kw["n_ctx"]] * kw["G"])


def test_the_calls_the_chain_batch_builds(monkeypatch):
    domain, trials, pool = chain_case(8, 3)
    calls = []
    monkeypatch.setattr(pool_mod, "_score_device", lambda *a, **kw: calls.append(
        ("score", a[3], a[4:], set(kw))) or ("eng", "mirror"))
    for name in ("_topk_device", "_liar_device"):
        monkeypatch.setattr(pool_mod, name, lambda *a, name=name: calls.append(
            (name, a)) or np.asarray([6, 2]))
    tpe.suggest_from_pool([100, 101], domain, trials, 0, pool=pool, joint="chain",
                          batch="liar-chain", lie_weight=2.0, verbose=False)
    (_s, st, rest, kws), (which, args) = calls
    assert rest == (False,) and kws == {"hist"}
    assert st.joint == dict(bandwidth=J.BANDWIDTH, cat_smoothing=J.CAT_SMOOTHING, tree="chain")
    assert (st.lie, st.lie_tree, st.lie_chain) == (2.0, False, True)
    assert (which, args) == ("_liar_device", ("eng", "mirror", 8, 2, None, 2.0, False, "chain"))
