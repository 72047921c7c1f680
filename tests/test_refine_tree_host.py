"""The climb of joint.py "Refining in a tree" on the host:
``joint.refine_tree_numpy`` against ``joint.refine_numpy``, and the argument
errors of ``refine_tree=``."""
import numpy as np
import pytest

from hyperopt_amd import Domain, hp, tpe
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from tests import joint_util as U
from tests.refine_tree_util import kinds_space, random_tree_case
from tests.refine_util import KW, all_kinds_case


def test_flat_space_has_the_bits_of_refine_numpy():
    domain, _trials, hist, vals = all_kinds_case()
    for refine in (0, 3):
        flat = J.refine_numpy(domain, hist, vals, refine, **KW)
        tree = J.refine_tree_numpy(domain, hist, vals, refine, **KW)
        assert tree[0].tobytes() == flat[0].tobytes() and tree[3].tobytes() == flat[3].tobytes()
        for a, b in zip(tree[1:], flat[1:]):
            assert a.reshape(b.shape).tobytes() == b.tobytes()
    same = J.refine_tree_numpy(domain, hist, vals, 0, **KW)[0]
    assert same.tobytes() == vals.tobytes() != tree[0].tobytes() and same is not vals


def test_conditional_space_root_columns_and_ascent():
    domain, _trials, hist, vals = random_tree_case(kinds_space(), 150, 32, 3)
    labels = list(domain.params)
    out, J0, J1, g, acc = J.refine_tree_numpy(domain, hist, vals, 4, **KW)
    assert J.refine_tree_numpy(domain, hist, vals, 0, **KW)[0].tobytes() == vals.tobytes()
    groups = [grp.labels for grp in J.joint_groups(domain)]
    assert groups == [["s", "x", "y"], ["alu", "aq", "au", "n"], ["aln", "an"], ["br"]]
    live = np.stack([~np.isnan(vals[:, labels.index(labs[0])]) for labs in groups], 1)
    assert live.all(0).tolist() == [True, False, False, False] and live.any(0).all()
    assert (np.isnan(J0) == ~live).all() and (np.isnan(J1) == ~live).all() and not acc[~live].any()
    assert g.shape == (32, 6) and np.isnan(g[~live[:, 1], 2:4]).all() and not acc[:, 3].any()
    assert (np.nansum(J1, 1) >= np.nansum(J0, 1)).all() and (J1[live] >= J0[live]).all()
    assert acc[:, :3][live[:, :3]].any() and (np.isnan(out) == np.isnan(vals)).all()
    # the root fit is the joint=True fit: the root columns are refine_numpy's
    root = [labels.index(lab) for lab in groups[0]]
    flat = J.refine_numpy(domain, hist, np.nan_to_num(vals), 4, **KW)
    assert out[:, root].tobytes() == flat[0][:, root].tobytes()
    assert J1[:, 0].tobytes() == flat[2].tobytes() and acc[:, 0].tobytes() == flat[4].tobytes()
    # quantized and discrete labels, and the selectors, stay
    fixed = [labels.index(lab) for lab in ("s", "aq", "n", "br")]
    assert out[:, fixed].tobytes() == vals[:, fixed].tobytes()


def test_argument_errors():
    domain, trials, _hist, vals = random_tree_case(kinds_space(), 30, 4, 5)
    sug = lambda **kw: tpe.suggest_sampled([0], domain, trials, 0, **kw)  # noqa: E731
    for bad in (-1, 2.0, "3", True):
        for call in (lambda: sug(joint="tree", refine_tree=bad),
                     lambda: tpe.refine_configs(domain, trials, vals, bad, joint="tree")):
            with pytest.raises(ValueError, match="refine_tree="):
                call()
    with pytest.raises(ValueError, match="refine= .* needs joint=True.*refine_tree"):
        sug(joint="tree", refine=4)
    for joint in (False, True):
        with pytest.raises(ValueError, match="refine_tree= .* needs joint='tree'"):
            sug(joint=joint, refine_tree=4)
    with pytest.raises(ValueError, match="refine_tree= .*coupled through their contexts"):
        sug(joint="chain", refine_tree=4)
    with pytest.raises(ValueError, match="joint=True or joint='tree'"):
        tpe.refine_configs(domain, trials, vals, 2, joint="chain")
    pool = tpe.Pool.from_arrays(domain, vals, ~np.isnan(vals))
    with pytest.raises(ValueError, match="refine_tree= .*closed set"):
        tpe.suggest_from_pool([0], domain, trials, 0, pool=pool, joint="tree", refine_tree=4)
    flat = Domain(lambda x: 0, {"x": hp.uniform("x", 0, 1), "y": hp.uniform("y", 0, 1)})
    none = U.make_trials(flat, [], [])
    with pytest.raises(ValueError, match="refine_tree= .*pass one of the two"):
        tpe.suggest_sampled([0], flat, none, 0, joint="tree", refine=2, refine_tree=2)
    grid = tpe.GridPool(flat, {"x": [0.1, 0.5], "y": [0.2, 0.7]}, joint=True)
    with pytest.raises(ValueError, match="refine_tree= .*GridPool"):
        tpe.suggest_from_pool([0], flat, none, 0, pool=grid, joint="tree", refine_tree=4)
    n = J._L.REFINE_MAX_CONT + 1  # one continuous label too many inside a branch
    wide = Domain(lambda x: 0, {"s": hp.choice("s", [
        {"x%02d" % i: hp.uniform("x%02d" % i, 0, 1) for i in range(n)}, {}])})
    none, row = U.make_trials(wide, [], []), np.full((1, n + 1), 0.5)
    row[0, list(wide.params).index("s")] = 0.0
    hist = tpe.collect_history(none, list(wide.params))
    for call in (lambda: J.refine_tree_numpy(wide, hist, row, 1),
                 lambda: tpe.refine_configs(wide, none, row, 1, joint="tree"),
                 lambda: tpe.suggest_sampled([0], wide, none, 0, joint="tree", refine_tree=1)):
        with pytest.raises(ValueError, match="at most %d" % (n - 1)):
            call()


def test_refine_tree_none_builds_the_calls_it_always_built(monkeypatch):
    """``refine_tree=None`` (and 0): ``_sample``, ``_pick`` and ``take_rows`` with
    the arguments of the code before ``refine_tree`` existed, never the climb."""
    domain, trials, _hist, vals = random_tree_case(kinds_space(), 30, 2, 5)
    calls = []

    class _Pool(object):
        n_untaken, vals, __len__ = 8, None, lambda self: 8
        mark_taken = lambda self, rows: calls.append(("taken", list(rows)))  # noqa: E731

    _Dev = type("_Dev", (), dict(rows_out="the rows on the device"))

    def step(name, result):
        def run(*args, **kw):
            calls.append((name, args, kw))
            return result
        return run

    def no_climb(*args, **kw):
        raise AssertionError("refine_tree=None reached the climb")

    monkeypatch.setattr(pool_mod, "_sample", step("sample", _Pool()))
    monkeypatch.setattr(pool_mod, "_pick", step("pick", np.asarray([6, 2], np.int64)))
    monkeypatch.setattr(pool_mod, "take_rows", step("take", (vals, ~np.isnan(vals))))
    for mod, name, f in ((pool_mod, "_mirror", lambda pool, eng: _Dev),
                         (tpe, "engine", lambda: "eng"), (pool_mod, "_refine_rows", no_climb),
                         (J, "refine_tree_device", no_climb), (J, "refine_device", no_climb)):
        monkeypatch.setattr(mod, name, f)
    for kw in (dict(), dict(refine_tree=None), dict(refine_tree=0)):
        del calls[:]
        docs = tpe.suggest_sampled([100, 101], domain, trials, 3, n_EI_candidates=8, joint="tree",
                                   draw="joint", verbose=False, **dict(KW, **kw))
        assert len(docs) == 2 and [c[0] for c in calls] == ["sample", "pick", "take", "taken"]
        (_, args, skw), st = calls[0], calls[0][1][4]
        assert args[:4] == (domain, trials, 3, 8) and args[5] is False and set(skw) == {"hist"}
        assert (st.prior_weight, st.gamma, st.lf, st.lie, st.refine, st.refine_tree) == \
            (0.7, 0.3, 25, None, 0, 0)
        assert st.joint == dict(bandwidth=0.25, cat_smoothing=0.5, tree=True)
        pargs = calls[1][1]
        assert pargs[0] == "eng" and pargs[2] is _Dev and pargs[3] == 2 and pargs[5] is False
        assert pargs[6] is st and len(pargs) == 7 and not calls[1][2]
        assert calls[2][1][1:] == ("the rows on the device", 2)
