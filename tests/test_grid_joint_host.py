"""The joint criterion on a GridPool, on the host (no GPU): the per-block plan
(``tpe.grid_joint_plan``), what ``GridPool(joint=True)`` refuses, and the
argument checks of tpe_grid_joint_factors / tpe_grid_joint_score /
tpe_grid_fold_onto that come before any launch."""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import Domain, hp, tpe
from hyperopt_amd import _lib as L
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from tests import joint_tree_util as TU
from tests import joint_util as U
from tests.test_grid_pool_host import FLAT, FLAT_AXES, NESTED_AXES

BRANCH_AXES = {"v": [1, 0], "a": [3, 0, 1, 2], "b": [0, 1, 2, 3], "c": [0.5, 0.25, 0.75]}


def _domain(space):
    return Domain(lambda x: 0, space)


def _check_plan(grid, plan, groups):
    """The plan's statements, from the grid's own blocks: which labels of a
    block are a group's, the F row of digit 0, the radices, the live groups."""
    labels = grid.labels
    assert [[labels[j] for j in cols] for cols in plan.groups] == groups
    for g, cols in enumerate(plan.groups):
        at = 0
        for j in cols:  # a group's axes follow one another in label order
            assert plan.axis_row[g][j] == at
            at += grid.axes[j].size
        assert plan.n_frows[g] == at
    assert len(plan.blocks) == len(grid.blocks)
    for b, blk in zip(grid.blocks, plan.blocks):
        assert blk.radix.dtype == np.int64 and blk.radix.tolist() == b.radix.tolist()
        for g, cols in enumerate(plan.groups):
            first_in = cols[0] in b.cols.tolist()
            assert blk.live[g] == first_in
            if not first_in:
                assert blk.frow[g] is None and blk.joint[g] == []
                assert not set(cols) & set(b.cols.tolist())
                continue
            assert [int(b.cols[i]) for i in blk.joint[g]] == cols
            frow = blk.frow[g]
            assert frow.dtype == np.int64 and frow.shape == b.cols.shape
            for i, j in enumerate(b.cols.tolist()):
                if j in cols:
                    assert frow[i] == plan.axis_row[g][j] + b.pos[i]
                    assert frow[i] + b.radix[i] <= plan.axis_row[g][j] + grid.axes[j].size
                else:
                    assert frow[i] == -1
        assert blk.live[0]


def test_plan_of_a_flat_space():
    d = _domain(FLAT)
    grid = tpe.GridPool(d, FLAT_AXES, joint=True)
    plan = grid.joint_plan()
    assert plan is grid.joint_plan(False)  # made once
    _check_plan(grid, plan, [list(d.params)])
    # "c" is a choice: one block per value, the selector fixed at radix 1 and
    # its F row moved to the block's value
    ci = grid.labels.index("c")
    assert len(grid.blocks) == 3
    for k, (b, blk) in enumerate(zip(grid.blocks, plan.blocks)):
        i = b.cols.tolist().index(ci)
        assert b.radix[i] == 1 and blk.frow[0][i] == plan.axis_row[0][ci] + k
        assert (blk.frow[0] >= 0).all()  # every label is joint
    tree = grid.joint_plan("tree")
    _check_plan(grid, tree, [list(d.params)])
    assert tpe.grid_joint_plan is pool_mod.grid_joint_plan


def test_plan_of_the_branch_space():
    d = _domain(TU.branch_space())
    grid = tpe.GridPool(d, BRANCH_AXES, joint=True)
    _check_plan(grid, grid.joint_plan(), [["v"]])
    for blk in grid.joint_plan().blocks:  # v first, everything else decode-only
        assert blk.frow[0][0] >= 0 and (blk.frow[0][1:] == -1).all()
    plan = grid.joint_plan(tree=True)
    groups = [g.labels for g in J.joint_groups(d)]
    assert groups == [["v"], ["a", "b"], ["c"]]
    _check_plan(grid, plan, groups)
    # the axis of v is [1, 0]: block 0 is branch 1 (c); a and b are choices, so
    # branch 0 is one block of one row per (a, b), both fixed at radix 1
    assert [blk.live for blk in plan.blocks] == [[True, False, True]] + 16 * [[True, True, False]]
    assert [b.rows for b in grid.blocks] == [3] + 16 * [1]
    assert plan.blocks[0].frow[0].tolist() == [0, -1]
    assert plan.blocks[0].frow[2].tolist() == [-1, 0]
    for k, blk in enumerate(plan.blocks[1:]):
        assert blk.radix.tolist() == [1, 1, 1]
        assert blk.frow[0].tolist() == [1, -1, -1]
        assert blk.frow[1].tolist() == [-1, k // 4, 4 + k % 4]


def test_plan_of_the_nested_case():
    d = TU.nested_case()[0]
    grid = tpe.GridPool(d, NESTED_AXES, joint=True)
    _check_plan(grid, grid.joint_plan(), [["root"]])
    plan = grid.joint_plan("tree")
    _check_plan(grid, plan, [g.labels for g in J.joint_groups(d)])
    # every group but the root's is live in some blocks only
    for g in range(1, len(plan.groups)):
        live = [blk.live[g] for blk in plan.blocks]
        assert any(live) and not all(live)


def test_plan_with_a_label_that_only_decodes_between_two_joint_ones():
    space = {"x": hp.uniform("x", 0, 1),
             "s": hp.choice("s", [{"y": hp.quniform("y", 0, 8, 2)}, {"w": hp.normal("w", 0, 1)}]),
             "z": hp.randint("z", 4)}
    d = _domain(space)
    axes = {"x": [0.1, 0.9], "s": [0, 1], "y": [0.0, 2.0, 8.0], "w": [-1.0, 0.5], "z": [3, 1, 0]}
    grid = tpe.GridPool(d, axes, joint=True)
    plan = grid.joint_plan()
    _check_plan(grid, plan, [J.joint_labels(d)])
    assert sorted(J.joint_labels(d)) == ["s", "x", "z"]
    between = 0
    for blk in plan.blocks:
        f = blk.frow[0].tolist()
        on = [i for i, v in enumerate(f) if v >= 0]
        between += sum(1 for v in f[on[0]:on[-1]] if v == -1)
    assert between > 0
    _check_plan(grid, grid.joint_plan("tree"), [g.labels for g in J.joint_groups(d)])


def test_refusals():
    d = _domain(FLAT)
    grid = tpe.GridPool(d, FLAT_AXES, joint=True)
    with pytest.raises(ValueError, match="distinct"):
        tpe.suggest_from_pool([0], d, None, 0, pool=grid, distinct=True, joint=True)
    with pytest.raises(ValueError, match="bandwidth"):
        tpe.score_configs(d, None, grid, joint=True, bandwidth=0.0)
    # a space without a label that is live in every configuration: at construction
    with pytest.raises(ValueError, match="live in every configuration"):
        tpe.GridPool(_domain({"x": 1.0}), {}, joint=True)
    tpe.GridPool(_domain({"x": 1.0}), {})  # (without the plan it is a grid of one row)
    # "tree" on a space whose switch is not selected by a bare label
    from hyperopt_amd.pyll import scope
    a, b = hp.randint("a", 2), hp.randint("b", 2)
    sw = _domain(scope.switch(a + b, hp.uniform("x", 0, 1), hp.uniform("y", 0, 1),
                              hp.uniform("z", 0, 1)))
    axes = {"a": [0, 1], "b": [0, 1], "x": [0.5], "y": [0.5], "z": [0.5]}
    g2 = tpe.GridPool(sw, axes, joint=True)  # (joint=True has its labels: a and b)
    assert [g2.labels[j] for j in g2.joint_plan().groups[0]] == ["a", "b"]
    with pytest.raises(ValueError, match="switch"):
        g2.joint_plan("tree")
    with pytest.raises(ValueError, match="switch"):
        tpe.score_configs(sw, None, g2, joint="tree")
    with pytest.raises(ValueError, match="another space"):
        tpe.score_configs(_domain(TU.branch_space()), None, grid, joint=True)


def test_a_grid_built_without_joint_still_raises():
    d = _domain(FLAT)
    for grid in (tpe.GridPool(d, FLAT_AXES), tpe.GridPool(d, FLAT_AXES, joint=False),
                 tpe.GridPool(d, FLAT_AXES, None, 0)):
        assert grid.joint is False
        for joint in (True, "tree"):
            with pytest.raises(ValueError, match="to_pool"):
                tpe.score_configs(d, None, grid, joint=joint)
            with pytest.raises(ValueError, match="joint=True"):
                tpe.suggest_from_pool([0], d, None, 0, pool=grid, joint=joint, verbose=False)
        with pytest.raises(ValueError, match="to_pool"):
            grid.joint_plan()
    assert tpe.GridPool(d, FLAT_AXES, joint=1).joint is True


# -- the C entries ---------------------------------------------------------------
def _layout():
    lib = L.load()
    out = (ctypes.c_int64 * 4)()
    assert lib.tpe_grid_joint_layout(ctypes.cast(out, ctypes.c_void_p), 4) == 4
    return tuple(out)


def test_layout_and_struct_sizes():
    lib = L.load()
    tile, chunk, per, limit = _layout()
    assert chunk == lib.tpe_joint_chunk() == 256 and per == 8 and chunk % per == 0
    assert tile >= 1 and limit == L.COND_MAX_LABELS
    two = (ctypes.c_int64 * 2)(-1, -1)
    assert lib.tpe_grid_joint_layout(ctypes.cast(two, ctypes.c_void_p), 2) == 2
    assert tuple(two) == (tile, chunk)
    assert lib.tpe_grid_joint_layout(None, 0) == 0
    assert lib.tpe_grid_joint_scratch_bytes(10, 0) == 160
    assert lib.tpe_grid_joint_scratch_bytes(10, 255) == 160
    assert lib.tpe_grid_joint_scratch_bytes(10, 256) == 320
    assert lib.tpe_grid_joint_scratch_bytes(-1, 4) == -1
    assert lib.tpe_grid_joint_scratch_bytes(4, -1) == -1
    # additive: the version and the struct mirrors are what they were
    assert lib.tpe_abi_version() == L.ABI_VERSION == 22
    sizes = (ctypes.c_int32 * 11)()
    lib.tpe_struct_sizes(ctypes.cast(sizes, ctypes.c_void_p), 11)
    assert tuple(sizes) == (L.SEG_DTYPE.itemsize, L.CAT_SEG_DTYPE.itemsize, L.JOB_DTYPE.itemsize,
                            L.BEST_DTYPE.itemsize, L.TABLE_DTYPE.itemsize, L.GATHER_DTYPE.itemsize,
                            L.HISTORY_DTYPE.itemsize, L.PRIOR_DTYPE.itemsize, L.OP_DTYPE.itemsize,
                            L.BAND_DTYPE.itemsize, L.COLSPEC_DTYPE.itemsize)
    one = (ctypes.c_int32 * 1)()
    lib.tpe_joint_struct_sizes(ctypes.cast(one, ctypes.c_void_p), 1)
    assert one[0] == L.JOINT_LABEL_DTYPE.itemsize


def test_score_checks_arguments():
    lib = L.load()
    tile, chunk, _per, limit = _layout()
    one = ctypes.c_void_p(16)  # a non-null stand-in: validation fails before any launch
    radix = np.array([4, 1, 5], np.int64)
    frow = np.array([0, -1, 4], np.int64)

    def score(F=one, ldF=chunk, n_frows=9, comp_begin=0, n_comp=chunk, dset=one, n=10,
              radp=radix.ctypes.data, frp=frow.ctypes.data, n_labels=3, row_begin=0, n_rows=20,
              sub=None, out=one, mode=L.GRID_JOINT_STORE, scratch=one, last=1):
        return lib.tpe_grid_joint_score(F, ldF, n_frows, comp_begin, n_comp, dset, n, radp, frp,
                                        n_labels, row_begin, n_rows, sub, out, mode, scratch, last,
                                        None)

    assert score(n_rows=0) == 0 and score(row_begin=20, n_rows=0) == 0  # nothing to do
    assert score(n_rows=0, F=None, dset=None, out=None, scratch=None) == 0
    for kw in (dict(F=None), dict(dset=None), dict(out=None), dict(scratch=None), dict(radp=None),
               dict(frp=None)):
        assert score(**kw) == -1 and b"null" in lib.tpe_last_error(), kw
    assert b"tpe_grid_joint_score" in lib.tpe_last_error()
    assert score(n_rows=-1) == -1 and score(row_begin=-1) == -1
    assert score(n_rows=21) == -1 and b"leave the block" in lib.tpe_last_error()
    assert score(row_begin=15, n_rows=6) == -1
    # the component window: whole chunks, inside ldF, beginning at a component
    for kw in (dict(n_comp=chunk - 1), dict(n_comp=chunk + 8, ldF=2 * chunk), dict(n_comp=0),
               dict(comp_begin=8), dict(comp_begin=-chunk), dict(comp_begin=chunk),
               dict(n_comp=2 * chunk), dict(ldF=chunk + 1, n_comp=chunk), dict(n=-1)):
        assert score(**kw) == -1 and b"whole chunks" in lib.tpe_last_error(), kw
    # `last` must say whether the window holds the set's last component
    assert score(last=0) == -1 and b"last=0" in lib.tpe_last_error()
    assert score(n=chunk, last=1) == -1 and b"last=1" in lib.tpe_last_error()
    assert score(n=chunk, last=0, n_rows=0) == 0
    assert score(n=chunk, comp_begin=chunk, last=1, n_rows=0) == 0
    for mode in (-1, 2, 3):
        assert score(mode=mode) == -1 and b"out_mode" in lib.tpe_last_error()
    assert score(mode=L.GRID_JOINT_ADD, n_rows=0) == 0
    # radices and F rows
    for bad in (0, -2):
        radix[1] = bad
        assert score() == -1 and b"label 1: radix" in lib.tpe_last_error()
    radix[1] = 1
    assert score(n_frows=8) == -1 and b"label 2: F rows" in lib.tpe_last_error()
    assert score(n_frows=2 ** 31) == -1
    none = np.full(3, -1, np.int64)
    assert score(frp=none.ctypes.data) == -1 and b"no joint label" in lib.tpe_last_error()
    # the label limit
    many, zeros = np.ones(limit + 1, np.int64), np.zeros(limit + 1, np.int64)
    assert score(n_labels=limit, n_rows=0, radp=many.ctypes.data, frp=zeros.ctypes.data) == 0
    assert score(n_labels=limit + 1, n_rows=0, radp=many.ctypes.data,
                 frp=zeros.ctypes.data) == L.E_UNSUPPORTED
    assert b"at most" in lib.tpe_last_error()
    assert score(n_labels=0) == -1 and score(n_labels=-1) == -1


def test_factors_check_arguments():
    lib = L.load()
    _tile, chunk, _per, limit = _layout()
    one = ctypes.c_void_p(16)
    host = np.zeros(limit + 1, L.JOINT_LABEL_DTYPE)
    host["kind"], host["col"] = L.JOINT_CONT, 0
    off, length, frow = (np.array(v, np.int64) for v in ([0, 3], [3, 2], [0, 3]))

    def factors(labels=one, n_labels=2, tables=None, n_tables=0, dset=one, n=10, axes=one,
                n_axes=5, offp=off.ctypes.data, lenp=length.ctypes.data, frp=frow.ctypes.data,
                F=one, ldF=chunk, n_frows=5, comp_begin=0, n_comp=chunk):
        return lib.tpe_grid_joint_factors(host.ctypes.data, labels, n_labels, tables, n_tables,
                                          dset, n, axes, n_axes, offp, lenp, frp, F, ldF, n_frows,
                                          comp_begin, n_comp, None)

    for kw in (dict(labels=None), dict(dset=None), dict(axes=None), dict(F=None), dict(offp=None),
               dict(lenp=None), dict(frp=None)):
        assert factors(**kw) == -1 and b"null pointer" in lib.tpe_last_error(), kw
    assert b"tpe_grid_joint_factors" in lib.tpe_last_error()
    for kw in (dict(n_comp=chunk - 1), dict(n_comp=0), dict(comp_begin=8), dict(comp_begin=chunk),
               dict(ldF=chunk - 2), dict(n=-1)):
        assert factors(**kw) == -1 and b"whole chunks" in lib.tpe_last_error(), kw
    assert factors(n_axes=4) == -1 and b"label 1: axis" in lib.tpe_last_error()
    assert factors(n_frows=4) == -1 and b"label 1: axis" in lib.tpe_last_error()
    assert factors(n_labels=0) == -1
    assert factors(n_labels=limit + 1) == L.E_UNSUPPORTED
    host["kind"][1] = 7
    assert factors() == -1 and b"label 1" in lib.tpe_last_error()
    host["kind"][1] = L.JOINT_CAT
    host["n_cat"][1] = 3
    assert factors(tables=one, n_tables=8) == -1       # its tables end at 9 of 8
    assert factors(tables=None, n_tables=9) == -1 and b"null pointer" in lib.tpe_last_error()
    host["n_cat"][1] = L.JOINT_MAX_CAT + 1
    assert factors(tables=one, n_tables=10 ** 6) == L.E_UNSUPPORTED


def test_fold_onto_checks_arguments():
    """tpe_grid_fold's checks under its own name; an offset < 0 is no error."""
    lib = L.load()
    one = ctypes.c_void_p(8)
    off = np.array([0, -1, 3], np.int64)
    radix = np.array([4, 1, 5], np.int64)

    def fold(n_labels=3, row_begin=0, n_rows=20, bl=one, al=one, S=one, offp=off.ctypes.data,
             radp=radix.ctypes.data):
        return lib.tpe_grid_fold_onto(bl, al, offp, radp, n_labels, row_begin, n_rows, S, None)

    assert fold(n_rows=0) == 0 and fold(row_begin=20, n_rows=0) == 0
    for kw in (dict(bl=None), dict(al=None), dict(S=None), dict(offp=None), dict(radp=None)):
        assert fold(**kw) == -1 and b"null pointer" in lib.tpe_last_error(), kw
    assert b"tpe_grid_fold_onto" in lib.tpe_last_error()
    assert fold(n_rows=-1) == -1 and b"n_rows=-1" in lib.tpe_last_error()
    assert fold(n_rows=21) == -1 and b"leave the block" in lib.tpe_last_error()
    assert fold(n_labels=1000, n_rows=1) == -1
    radix[1] = 0
    assert fold() == -1 and b"tpe_grid_fold_onto: label 1 has radix" in lib.tpe_last_error()
    radix[1] = 1
    assert lib.tpe_grid_fold(None, None, off.ctypes.data, radix.ctypes.data, 3, 0, 1, one,
                             None) == -1
    assert b"tpe_grid_fold: null pointer" in lib.tpe_last_error()


def test_all_kinds_space_needs_no_device_for_its_plan():
    d = _domain(U.all_kinds_space(hp))
    axes = {"a": [0, 1, 2], "b": [0, 9], "bb": [12, 24], "c": [4.0, 7.0], "d": [0.2, 1.0],
            "e": [0.0, 9.0], "f": [2.0, 20.0], "g": [-3.0, 4.0], "h": [0.1, 5.0],
            "i": [-2.0, 8.0], "j": [0.0, 3.0], "k": [1, 2]}
    grid = tpe.GridPool(d, axes, joint=True)
    _check_plan(grid, grid.joint_plan(), [list(d.params)])
    assert grid._device == {}
