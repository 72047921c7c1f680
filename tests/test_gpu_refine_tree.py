"""tpe_joint_refine_tree on the device against ``joint.refine_tree_numpy``.

Tolerances are the reference's own, per group (``refine_tree_numpy(
return_info=True)``; tests/test_gpu_refine.py): ``J_bound`` on J, ``g_bound`` on
g and ``t_bound`` on the point reached.  Accepted counts are compared exactly:
a case's rows are the first of a seeded draw every decision of which, in every
live group, the reference alone shows to have |J(t') - J(t)| >= 100 x the bound
(``refine_tree_util.safe_tree_rows``), and ``_run`` asserts that of every row.
"""
import numpy as np
import pytest

from hyperopt_amd import hp, tpe
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from tests.refine_tree_util import (kinds_space, random_tree_case, safe_tree_rows, tree_case)
from tests.refine_util import KW

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
SENTINEL = 12345.0  # what the cells of labels not live in a row hold at the C ABI


def _device(domain, hist, vals, kw, joint="tree"):
    st = pool_mod._settings(kw["prior_weight"], kw["gamma"], 25, joint, kw["bandwidth"],
                            kw["cat_smoothing"])
    eng, active = tpe.engine(), ~np.isnan(vals)
    d = tpe.Pool.from_arrays(domain, vals, active).device(eng)
    dead = eng.torch.from_numpy(np.ascontiguousarray(~active.T)).to(eng.device)
    d.vals[:, :vals.shape[0]][dead] = SENTINEL
    return eng, d, pool_mod._fit(eng, domain, hist, vals.shape[1], st)


def _run(domain, hist, vals, refine, kw=KW):
    ref, J0, J1, g, acc, info = J.refine_tree_numpy(domain, hist, vals, refine, return_info=True,
                                                    **kw)
    assert not (info["margin"] < 100.0).any()
    (P, L), active = vals.shape, ~np.isnan(vals)
    eng, d, fits = _device(domain, hist, vals, kw)
    tr, before = {}, d.vals[:, :P].cpu().numpy().T
    J.refine_tree_device(fits, d.vals, d.active, d.vals.shape[1], L, P, refine, tr)
    tr = {k: v.cpu().numpy() for k, v in tr.items()}
    got = d.vals[:, :P].cpu().numpy().T
    cont = [[m for m in f.dj.models if m.kind == J._L.JOINT_CONT] for f in fits]
    rest = [j for j in range(L) if j not in [m.col for c in cont for m in c]]
    assert got[:, rest].tobytes() == before[:, rest].tobytes()  # (no other column is written)
    assert (got[~active] == SENTINEL).all()  # (a label not live in the row: never written)
    np.testing.assert_array_equal(tr["accepted"], acc)
    for name, want in (("J_start", J0), ("J_end", J1), ("g_end", g)):  # (dead pairs: NaN)
        np.testing.assert_array_equal(np.isnan(tr[name]), np.isnan(want))
    still = acc.sum(1) == 0
    assert got[still].tobytes() == before[still].tobytes()  # (no step kept: no bit moved)
    off = np.concatenate([[0], np.cumsum([len(c) for c in cont])])
    for gi, ms in enumerate(cont):
        sl, fin = slice(off[gi], off[gi + 1]), np.isfinite(J0[:, gi])
        tb = info["t_bound"][:, sl]
        assert (np.abs(tr["J_start"] - J0)[fin, gi] <= info["J_bound"][fin, gi]).all()
        # (the end points differ by t_bound: J by |g| t_bound, g by K t_bound on top)
        assert (np.abs(tr["J_end"] - J1)[fin, gi] <=
                (info["J_bound"][:, gi] + (np.abs(g[:, sl]) * tb).sum(1))[fin]).all()
        slack = np.einsum("pde,pe->pd", info["K"][gi], tb)
        assert (np.abs(tr["g_end"] - g)[:, sl][fin] <= (info["g_bound"][:, sl] + slack)[fin]).all()
        for j, m in enumerate(ms):
            td, tw = J._fit(m, got[fin, m.col]), J._fit(m, ref[fin, m.col])
            assert (np.abs(td - tw) <= tb[fin, j] + 4 * EPS * (np.abs(tw) + 1)).all()
    return tr, got


@pytest.mark.parametrize("refine", [0, 3])
def test_every_kind_and_dead_pairs(refine):
    domain, _trials, hist, cand = random_tree_case(kinds_space(), 150, 64, 3)
    vals = safe_tree_rows(domain, hist, cand, refine, 16)
    live = ~np.isnan(vals[:, [list(domain.params).index(lab) for lab in ("s", "au", "an", "br")]])
    assert (~live).any(0).tolist() == [False, True, True, True] and live.any(0).all()
    tr, _got = _run(domain, hist, vals, refine)
    assert not tr["accepted"][~live].any() and np.isnan(tr["J_end"][~live]).all()
    assert (refine == 0) == (not tr["accepted"].any())
    assert not tr["accepted"][:, 3].any() and np.isfinite(tr["J_start"][live[:, 3], 3]).all()


def _branch_labels(prefix):
    """Eight labels, three of them continuous: E = 380 staged components."""
    names = [prefix + c for c in "abcdefgh"]
    return dict(zip(names, [
        hp.uniform(names[0], 0, 1), hp.normal(names[1], 0, 1), hp.loguniform(names[2], -2, 1),
        hp.quniform(names[3], 0, 8, 2), hp.qnormal(names[4], 0, 2, 1), hp.randint(names[5], 3),
        hp.choice(names[6], [0, 1]), hp.choice(names[7], [0, 1, 2])]))


E8 = J._L.refine_stage_components(8)


@pytest.mark.parametrize("comps", [1, 2, 256, 257, E8, E8 + 1])
def test_above_set_size_edges(comps):
    """1: never tried; 256 / 257: the block's threads; E / E + 1: staged / streamed."""
    from hyperopt_amd import Domain, rand
    assert tpe.engine().lib.tpe_joint_refine_tree_stage_components(8) == E8 and E8 + 1 <= 600
    space = {"s": hp.choice("s", [_branch_labels("a"), {"c": hp.uniform("c", 0, 1)}])}
    domain, rng = Domain(lambda x: 0, space), np.random.RandomState(comps)
    configs, losses = [], []
    want0 = 0 if comps == 1 else 3 + comps - 1  # branch 0: 3 below, comps - 1 above; 80 in branch 1
    while len(configs) < want0 + 80:
        c = rand.sample_config(domain, rng)
        n0 = sum(1 for x in configs if x["s"] == 0)
        if c["s"] == 0 and n0 == want0:
            continue
        if c["s"] == 1 and len(configs) - n0 == 80:
            continue
        configs.append(c)
        rank = sum(1 for x in configs if x["s"] == c["s"])
        # (the rest of the below side comes from branch 1: its losses lie between)
        losses.append((0.001 * rank if rank <= 3 else 1.0 + rng.uniform()) if c["s"] == 0 else
                      0.5 + 0.001 * rank)
    kw = dict(KW, gamma=0.25)
    domain, _trials, hist, cand = tree_case(space, configs, losses, 32, 77, force={"s": 0})
    cols = [list(domain.params).index(lab) for lab in J.joint_groups(domain)[1].labels]
    sizes = [J.set_rows(hist, m, cols).size + 1 for m in J.split_sets(hist, kw["gamma"])]
    assert sizes == [1 if comps == 1 else 4, comps]
    tr, _got = _run(domain, hist, safe_tree_rows(domain, hist, cand, 2, 8, kw), 2, kw)
    assert np.isfinite(tr["J_end"][:, 1]).all() and np.isnan(tr["J_end"][:, 2]).all()


@pytest.mark.parametrize("T", [200, 600])
def test_flat_space_has_the_flat_kernels_bits(T):
    """tpe_joint_refine_tree == tpe_joint_refine on one block: the above set
    staged (under E) and streamed (over it)."""
    domain, _trials, hist, vals = random_tree_case(_branch_labels("a"), T, 16, 21)
    n_above = J.set_rows(hist, J.split_sets(hist, KW["gamma"])[1], list(range(8))).size
    assert (n_above + 1 <= E8) == (T == 200)
    out = []
    for tree in (False, True):
        eng, d, fits = _device(domain, hist, vals, KW, "tree" if tree else True)
        tr = {}
        args = (d.vals, d.vals.shape[1], 8, 16, 3, tr)
        if tree:
            J.refine_tree_device(fits, args[0], d.active, *args[1:])
        else:
            J.refine_device(fits[0], *args)
        out.append([d.vals[:, :16].cpu().numpy()] + [tr[k].cpu().numpy().ravel() for k in sorted(tr)])
    assert out[0][3].any()  # (accepted: something moved)
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()


def test_root_columns_and_row_subsets():
    domain, trials, _hist, vals = random_tree_case(kinds_space(), 150, 16, 3)
    labels = list(domain.params)
    out, Jb, Ja, acc, g = tpe.refine_configs(domain, trials, vals, 4, return_trace=True,
                                             joint="tree", **KW)
    flat = tpe.refine_configs(domain, trials, vals, 4, **KW)
    root = [labels.index(lab) for lab in ("x", "y", "s")]
    assert out[:, root].tobytes() == flat[:, root].tobytes() and acc.any(0)[:3].all()
    assert (np.isnan(out) == np.isnan(vals)).all() and Jb.shape == Ja.shape == acc.shape == (16, 4)
    assert (Ja[~np.isnan(Ja)] >= Jb[~np.isnan(Jb)]).all() and g.shape == (16, 6)
    part = tpe.refine_configs(domain, trials, vals[1::3], 4, joint="tree", **KW)
    assert part.tobytes() == out[1::3].tobytes()
    assert tpe.refine_configs(domain, trials, vals, 0, joint="tree", **KW).tobytes() == \
        vals.tobytes()


def test_three_instantiation_classes_in_one_call():
    """Groups with D_c = 1, 5 and 16: one call, three launches."""
    normals = lambda p, n: {p + "%02d" % i: hp.normal(p + "%02d" % i, 0, 1) for i in range(n)}  # noqa: E731
    space = {"r": hp.uniform("r", 0, 1), "s": hp.choice("s", [normals("f", 5), normals("w", 16)])}
    domain, _trials, hist, cand = random_tree_case(space, 120, 64, 7)
    # (far from every trial the two priors cancel and J is flat: start near good trials)
    best = np.asarray(hist.vals)[np.argsort(hist.losses)]
    labels, rng = list(domain.params), np.random.RandomState(1)
    for r in range(64):
        near = best[np.flatnonzero(best[:, labels.index("s")] == cand[r, labels.index("s")])[r % 2]]
        cand[r] = np.where(np.isnan(cand[r]), np.nan, near + 0.4 * rng.randn(len(labels)))
        cand[r, labels.index("s")], cand[r, labels.index("r")] = near[labels.index("s")], rng.uniform()
    tr, _got = _run(domain, hist, safe_tree_rows(domain, hist, cand, 2, 16), 2)
    assert tr["g_end"].shape == (16, 22) and tr["accepted"].any(0).all()


@pytest.mark.parametrize("batch", [None, "liar-tree"])
def test_public_path_ridge_inside_a_branch(batch):
    """The loss is small only on y = x under option 0; the picks climb onto it."""
    space = {"v": hp.choice("v", [{"x": hp.uniform("x", 0, 1), "y": hp.uniform("y", 0, 1)},
                                  {"z": hp.uniform("z", 0, 1)}])}
    domain, trials, hist, _ = random_tree_case(
        space, 300, 0, 11, loss=lambda c: abs(c["x"] - c["y"]) if c["v"] == 0 else 1.0)
    labels = list(domain.params)
    kw = dict(KW, n_EI_candidates=256, joint="tree", draw="joint", verbose=False, batch=batch)

    def picks(**more):
        docs = tpe.suggest_sampled(range(900, 904), domain, trials, 9, **dict(kw, **more))
        return np.asarray([[d["misc"]["vals"][lab][0] if d["misc"]["vals"][lab] else np.nan
                            for lab in labels] for d in docs], float)

    plain, refined = picks(), picks(refine_tree=8)
    assert picks(refine_tree=0).tobytes() == plain.tobytes() and len(refined) == 4
    want = tpe.refine_configs(domain, trials, plain, 8, joint="tree", **KW)
    assert refined.tobytes() == want.tobytes() and refined.tobytes() != plain.tobytes()
    score = lambda v: tpe.score_configs(domain, trials, tpe.Pool.from_arrays(  # noqa: E731
        domain, v, ~np.isnan(v)), joint="tree", **KW)
    info = J.refine_tree_numpy(domain, hist, plain, 8, return_info=True, **KW)[5]
    w = int(np.argmax(score(refined)))
    assert score(refined)[w] - score(plain).max() > 100 * np.nansum(info["J_bound"][w])
