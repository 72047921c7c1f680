"""tpe.GridPool on the host (no GPU): the block and row enumeration against
itertools.product and the materialised Pool, axis validation, keep / exclude
and the taken bookkeeping, and the argument checks of tpe_grid_fold."""
import ctypes
import itertools

import numpy as np
import pytest

from hyperopt_amd import Domain, hp, tpe
from hyperopt_amd import _lib as L
from hyperopt_amd.pool import startup_rows
from tests.golden import spaces


def _domain(space):
    return Domain(lambda x: 0, spaces.SPACES[space](hp) if isinstance(space, str) else space)


FLAT = {"q": hp.quniform("q", 0, 40, 1), "u": hp.uniform("u", 0, 1),
        "c": hp.choice("c", ["x", "y", "z"]), "l": hp.loguniform("l", -3, 0)}
FLAT_AXES = {"q": [3.0, 0.0, 40.0, 7.5, 12.0], "u": [0.5, 0.25], "c": [2, 0, 1],
             "l": [0.1, 1.0, 0.3, 0.05]}
NESTED_AXES = {"root": [2, 0, 1], "lin_lr": [0.01, 0.5], "tree_depth": [1.0, 5.0, 12.0],
               "tree_split": [1, 0], "gini_w": [0.0, 0.5, 1.0], "ent_w": [-1.0, 2.0],
               "ent_s": [0.5, 1.0, 3.5], "nn_units": [8.0, 64.0], "nn_drop": [0.0, 0.35, 0.7]}
README_AXES = {"a": [0, 1], "c1": [0.5, 1.0, 4.0], "c2": [-10.0, 0.0, 3.0, 10.0]}


def _grids():
    return [("flat", _domain(FLAT), FLAT_AXES), ("nested", _domain("nested"), NESTED_AXES),
            ("readme", _domain("readme"), README_AXES)]


@pytest.mark.parametrize("name,domain,axes", _grids(),
                         ids=lambda v: v if isinstance(v, str) else "")
def test_rows_are_the_materialised_pool(name, domain, axes):
    g = tpe.GridPool(domain, axes)
    assert g.labels == list(domain.params)
    assert len(g) == sum(int(np.prod(b.radix)) for b in g.blocks) == int(g.block_off[-1])
    p = g.to_pool()  # (Pool's own validation: every block's label set is reachable()'s)
    assert len(p) == len(g) and p.labels == g.labels
    for r in range(len(g)):
        cfg = g.config(r)
        assert cfg == p.config(r), r
        assert list(cfg) == [lab for lab in g.labels if lab in cfg]  # domain.params order
        assert all(type(cfg[lab]) is type(p.config(r)[lab]) for lab in cfg)
    assert len({tuple(sorted(g.config(r).items())) for r in range(len(g))}) == len(g)
    with pytest.raises(IndexError):
        g.config(len(g))


def test_flat_order_is_itertools_product():
    d = _domain(FLAT)
    g = tpe.GridPool(d, FLAT_AXES)
    labels = list(d.params)
    rows = list(itertools.product(*[FLAT_AXES[lab] for lab in labels]))
    assert len(g) == len(rows) == 5 * 2 * 3 * 4
    # (a choice is a selector: one block per value of "c", the first label, so
    # the blocks in axis order are the product's slowest digit)
    assert labels[0] == "c" and [b.rows for b in g.blocks] == [40, 40, 40]
    for r, vals in enumerate(rows):
        assert g.config(r) == dict(zip(labels, vals))
    assert type(g.config(0)["c"]) is int and type(g.config(0)["q"]) is float


def test_block_order_and_sizes():
    d = _domain("nested")
    g = tpe.GridPool(d, NESTED_AXES)
    # depth first, selectors in domain.params order, axis values in axis order:
    # root = 2 (nn), root = 0 (lin), root = 1 (tree) with tree_split = 1, then 0
    sizes = [2 * 3, 2, 3 * 2 * 3, 3 * 3]
    assert [b.rows for b in g.blocks] == sizes and len(g) == sum(sizes)
    assert g.block_off.tolist() == [0, 6, 8, 26, 35]
    assert g.config(0) == {"root": 2, "nn_units": 8.0, "nn_drop": 0.0}
    assert g.config(5) == {"root": 2, "nn_units": 64.0, "nn_drop": 0.7}
    assert g.config(6) == {"root": 0, "lin_lr": 0.01}
    tree = g.config(8)
    assert tree["root"] == 1 and tree["tree_split"] == 1 and set(tree) == {
        "root", "tree_depth", "tree_split", "ent_w", "ent_s"}
    assert g.config(26)["tree_split"] == 0 and "gini_w" in g.config(26)
    # a block whose only live labels are selectors has exactly one row
    sp = hp.choice("s", [0, hp.uniform("x", 0, 1), hp.choice("t", [1, 2])])
    g = tpe.GridPool(Domain(lambda x: 0, sp), {"s": [0, 1, 2], "x": [0.1, 0.2, 0.3], "t": [1, 0]})
    assert [b.rows for b in g.blocks] == [1, 3, 1, 1]
    assert [g.config(r) for r in range(len(g))] == [
        {"s": 0}, {"s": 1, "x": 0.1}, {"s": 1, "x": 0.2}, {"s": 1, "x": 0.3},
        {"s": 2, "t": 1}, {"s": 2, "t": 0}]
    g.to_pool()
    # a label live in no block is not scored
    g = tpe.GridPool(Domain(lambda x: 0, sp), {"s": [0, 2], "x": [0.1, 0.2, 0.3], "t": [1]})
    assert [g.config(r) for r in range(len(g))] == [{"s": 0}, {"s": 2, "t": 1}]
    assert [g.labels[j] for j in g.scored] == [lab for lab in g.labels if lab != "x"]


def test_too_many_blocks():
    sp = {"s%d" % i: hp.choice("s%d" % i, [0, hp.uniform("x%d" % i, 0, 1)]) for i in range(13)}
    axes = {}
    for i in range(13):
        axes["s%d" % i] = [0, 1]
        axes["x%d" % i] = [0.5]
    with pytest.raises(ValueError, match="4096"):
        tpe.GridPool(Domain(lambda x: 0, sp), axes)
    del sp["s12"], axes["s12"], axes["x12"]
    assert len(tpe.GridPool(Domain(lambda x: 0, sp), axes).blocks) == 4096


def test_validation_errors_name_the_label():
    d = _domain("many_dists")
    good = {"a": [0, 2], "b": [3], "bb": [12, 24], "c": [4.0, 7.0], "d": [0.2, 1.0],
            "e": [0.0, 4.7], "f": [0.0, 2.0], "g": [-30.0], "h": [0.1], "i": [1.0], "j": [2.0],
            "k": [1, 0]}
    assert len(tpe.GridPool(d, good)) == 2 ** 7

    def bad(**changes):
        axes = dict(good)
        for lab, v in changes.items():
            if v is None:
                del axes[lab]
            else:
                axes[lab] = v
        return axes

    for changes, lab, pos, what in [
            (dict(c=[4.0, 5.0, 4.0]), "c", 2, "repeated"),
            (dict(a=[1, 0, 2, 0]), "a", 3, "repeated"),
            (dict(c=[5.0, 7.5]), "c", 1, "outside"),          # uniform(4, 7)
            (dict(bb=[12, 13, 25]), "bb", 2, "outside"),      # randint(12, 25): high excluded
            (dict(a=[3]), "a", 0, "outside"),                 # choice of 3
            (dict(k=[0, 1.5]), "k", 1, "whole"),              # a non-whole category
            (dict(b=[2.5]), "b", 0, "whole"),
            (dict(g=[1.0, float("nan")]), "g", 1, "finite"),
            (dict(h=[float("inf")]), "h", 0, "finite")]:
        with pytest.raises(ValueError) as e:
            tpe.GridPool(d, bad(**changes))
        msg = str(e.value)
        assert repr(lab) in msg and "position %d" % pos in msg and what in msg, msg
    for changes, lab, what in [(dict(e=None), "e", "missing"),
                               (dict(zzz=[1.0]), "zzz", "not a label"),
                               (dict(f=[]), "f", "empty"),
                               (dict(d=[[0.2, 0.3]]), "d", "one-dimensional"),
                               (dict(i=["x"]), "i", "not numbers")]:
        with pytest.raises(ValueError) as e:
            tpe.GridPool(d, bad(**changes))
        assert repr(lab) in str(e.value) and what in str(e.value), str(e.value)
    # -0.0 and 0.0 are one value; ranges and arrays are sequences
    with pytest.raises(ValueError, match="repeated"):
        tpe.GridPool(d, bad(e=[0.0, -0.0]))
    assert len(tpe.GridPool(d, bad(b=range(10), c=np.linspace(4, 7, 5)))) == 2 ** 6 * 10 * 5


def test_keep_sees_every_row_once(monkeypatch):
    from hyperopt_amd import pool as pool_mod
    d = _domain("nested")
    monkeypatch.setattr(pool_mod, "KEEP_CHUNK", 8)  # 35 rows: chunks cross the blocks
    seen = []

    def keep(cols):
        assert list(cols) == list(d.params)
        n = cols["root"].size
        assert 0 < n <= 8 and all(c.shape == (n,) and c.dtype == np.float64
                                  for c in cols.values())
        seen.append({k: v.copy() for k, v in cols.items()})
        return ~(cols["nn_drop"] > 0.5) & ~(cols["gini_w"] == 0.5)  # (NaN compares false)

    g = tpe.GridPool(d, NESTED_AXES, keep=keep)
    P = len(g)
    assert sum(s["root"].size for s in seen) == P == 35
    full = {lab: np.concatenate([s[lab] for s in seen]) for lab in d.params}
    for r in range(P):
        cfg = g.config(r)
        for lab in d.params:  # NaN exactly where the label is dead
            if lab in cfg:
                assert full[lab][r] == cfg[lab]
            else:
                assert np.isnan(full[lab][r])
    want = np.array([g.config(r).get("nn_drop", 0) > 0.5 or g.config(r).get("gini_w") == 0.5
                     for r in range(P)])
    assert want.sum() == 2 + 3 and g.excluded.dtype == np.uint8
    np.testing.assert_array_equal(g.excluded.astype(bool), want)
    assert g.n_untaken == P - 5
    with pytest.raises(ValueError, match="shape"):
        tpe.GridPool(d, NESTED_AXES, keep=lambda cols: np.ones(3, bool))


def test_bookkeeping_and_startup_rows():
    d = _domain(FLAT)
    g = tpe.GridPool(d, FLAT_AXES, keep=lambda cols: cols["q"] != 7.5)
    P = len(g)
    ex = np.flatnonzero(g.excluded)
    assert P == 120 and ex.size == 24 and g.n_untaken == 96
    assert g.taken.dtype == np.uint8 and not g.taken.any() and g.row_of == {}
    free = np.flatnonzero(g.excluded == 0)
    g.mark_taken([free[3], free[7], free[7]])
    g.row_of[100], g.row_of[101] = int(free[3]), int(free[7])
    assert g.n_untaken == 94
    g.release([free[3]])
    assert g.n_untaken == 95 and not g.taken[free[3]] and g.row_of == {101: int(free[7])}
    with pytest.raises(ValueError, match="excluded"):
        g.release([ex[0]])
    with pytest.raises(IndexError):
        g.mark_taken([P])
    g.mark_taken([ex[1]])  # taken and excluded: counted once
    assert g.n_untaken == 95
    g.exclude([free[0]])
    assert g.n_untaken == 94 and g.excluded[free[0]]
    # the startup rule over untaken and unexcluded rows
    avail = np.flatnonzero((g.taken == 0) & (g.excluded == 0))
    assert avail.size == 94
    a = startup_rows(g, 5, 10)
    np.testing.assert_array_equal(
        a, avail[np.random.RandomState(5).choice(avail.size, 10, replace=False)])
    assert sorted(startup_rows(g, 1, 500).tolist()) == avail.tolist()
    for seed in range(20):
        assert not g.excluded[startup_rows(g, seed, 30)].any()
    # without exclusions: the rows of the materialised pool under the same seed and taken set
    g2 = tpe.GridPool(d, FLAT_AXES)
    p2 = g2.to_pool()
    assert g2.excluded is None
    for q in (g2, p2):
        q.mark_taken(np.arange(0, P, 3))
    np.testing.assert_array_equal(startup_rows(g2, 9, 12), startup_rows(p2, 9, 12))
    # nothing left: no document and nothing scored (no GPU here)
    g2.mark_taken(np.arange(P))
    assert g2.n_untaken == 0 and startup_rows(g2, 1, 4).size == 0
    assert tpe.suggest_from_pool([0, 1], d, None, 0, pool=g2) == []
    with pytest.raises(ValueError, match="another space"):
        tpe.suggest_from_pool([0], _domain("readme"), None, 0, pool=g)


def test_grid_fold_checks_arguments():
    """tpe_grid_fold reports argument errors before any launch and returns 0
    when there is nothing to do (no GPU needed here)."""
    lib = L.load()
    one = ctypes.c_void_p(8)  # a non-null stand-in: validation fails before any launch
    off = np.zeros(3, np.int64)
    radix = np.array([4, 1, 5], np.int64)

    def fold(n_labels=3, row_begin=0, n_rows=20, bl=one, al=one, S=one, offp=off.ctypes.data,
             radp=radix.ctypes.data):
        return lib.tpe_grid_fold(bl, al, offp, radp, n_labels, row_begin, n_rows, S, None)

    assert fold(n_rows=0) == 0 and fold(n_rows=0, bl=None, al=None, S=None) == 0
    assert fold(row_begin=20, n_rows=0) == 0  # an empty window at the block's end
    for kw in (dict(bl=None), dict(al=None), dict(S=None), dict(offp=None), dict(radp=None)):
        assert fold(**kw) == -1 and b"null pointer" in lib.tpe_last_error(), kw
    assert fold(n_rows=-1) == -1 and b"n_rows=-1" in lib.tpe_last_error()
    assert fold(row_begin=-3) == -1 and b"row_begin=-3" in lib.tpe_last_error()
    assert fold(n_labels=-1) == -1 and b"n_labels=-1" in lib.tpe_last_error()
    for bad in (0, -2):
        radix[1] = bad
        assert fold() == -1 and b"label 1 has radix" in lib.tpe_last_error()
    radix[1] = 1
    # a window that leaves the block of 20 rows
    assert fold(n_rows=21) == -1 and b"leave the block" in lib.tpe_last_error()
    assert fold(row_begin=15, n_rows=6) == -1 and b"leave the block" in lib.tpe_last_error()
    assert fold(row_begin=21, n_rows=0) == -1
    assert fold(row_begin=2 ** 62, n_rows=2 ** 62) == -1
    # at least 64 labels per call; more than the entry takes is an error, as is
    # a block whose row count does not fit int64
    many = np.ones(1000, np.int64)
    zeros = np.zeros(1000, np.int64)
    assert fold(n_labels=64, n_rows=0, offp=zeros.ctypes.data, radp=many.ctypes.data) == 0
    assert fold(n_labels=1000, n_rows=1, offp=zeros.ctypes.data, radp=many.ctypes.data) == -1
    assert b"n_labels=1000" in lib.tpe_last_error()
    many[:7] = 2 ** 10
    assert fold(n_labels=7, n_rows=1, offp=zeros.ctypes.data, radp=many.ctypes.data) == -1
    assert b"overflows" in lib.tpe_last_error()
    many[6] = 1
    assert fold(n_labels=7, row_begin=2 ** 60 - 1, n_rows=0, offp=zeros.ctypes.data,
                radp=many.ctypes.data) == 0
