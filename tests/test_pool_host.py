"""tpe.Pool on the host (no GPU): validation, the two constructors, the taken
bookkeeping, and the argument checks of the pool entry points of the C ABI."""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import Domain, hp, rand, tpe
from hyperopt_amd import _lib as L
from hyperopt_amd.pool import startup_rows
from tests.golden import spaces


def _domain(name):
    return Domain(lambda x: 0, spaces.SPACES[name](hp))


def _draws(domain, n, seed=0):
    rng = np.random.RandomState(seed)
    return [rand.sample_config(domain, rng) for _ in range(n)]


def test_validation_errors_name_row_and_label():
    d = _domain("many_dists")
    good = _draws(d, 4)
    tpe.Pool(d, good)  # prior draws are valid

    def bad(row, **changes):
        cfgs = [dict(c) for c in good]
        for lab, v in changes.items():
            if v is None:
                del cfgs[row][lab]
            else:
                cfgs[row][lab] = v
        return cfgs

    for row, changes, lab, what in [
            (2, dict(c=None), "c", "missing"),            # a live label left out
            (1, dict(c=7.5), "c", "outside"),             # uniform(4, 7)
            (3, dict(d=1.5), "d", "outside"),             # loguniform(-2, 0): above exp(0)
            (0, dict(a=3), "a", "outside"),               # choice of 3: category >= K
            (2, dict(k=-1), "k", "outside"),              # pchoice
            (1, dict(bb=11), "bb", "outside"),            # randint(12, 25) below low
            (1, dict(bb=25), "bb", "outside"),            # ... high is excluded
            (3, dict(b=2.5), "b", "whole"),               # randint value not an integer
            (0, dict(g=float("nan")), "g", "finite"),
            (2, dict(h=float("inf")), "h", "finite")]:
        with pytest.raises(ValueError) as e:
            tpe.Pool(d, bad(row, **changes))
        msg = str(e.value)
        assert "row %d" % row in msg and repr(lab) in msg and what in msg, msg
    with pytest.raises(ValueError, match="not a label"):
        tpe.Pool(d, bad(0, zzz=1.0))
    # quantized values need not lie on the lattice, and may round across a bound
    tpe.Pool(d, bad(0, e=4.7, f=0.0))


def test_conditional_label_sets():
    d = _domain("nested")
    good = _draws(d, 40)
    assert len({frozenset(c) for c in good}) > 2  # rows differ in their live labels
    tpe.Pool(d, good)
    lin = next(c for c in good if c["root"] == 0)
    tree = next(c for c in good if c["root"] == 1)
    with pytest.raises(ValueError) as e:  # a dead label given
        tpe.Pool(d, [tree, dict(lin, nn_drop=0.3)])
    assert "row 1" in str(e.value) and "'nn_drop'" in str(e.value) and "not live" in str(e.value)
    with pytest.raises(ValueError) as e:  # a live label of the taken branch missing
        tpe.Pool(d, [{k: v for k, v in tree.items() if k != "tree_depth"}])
    assert "row 0" in str(e.value) and "'tree_depth'" in str(e.value)
    with pytest.raises(ValueError) as e:  # the selector itself missing
        tpe.Pool(d, [lin, {k: v for k, v in lin.items() if k != "root"}])
    assert "row 1" in str(e.value)


@pytest.mark.parametrize("space", ["nested", "many_dists"])
def test_configs_and_arrays_agree(space):
    d = _domain(space)
    cfgs = _draws(d, 64, seed=3)
    p = tpe.Pool(d, cfgs)
    labels = list(d.params)
    vals = np.full((len(cfgs), len(labels)), -123.0)  # inactive entries are ignored
    active = np.zeros(vals.shape, bool)
    for r, c in enumerate(cfgs):
        for lab, v in c.items():
            vals[r, labels.index(lab)] = v
            active[r, labels.index(lab)] = True
    q = tpe.Pool.from_arrays(d, vals, active)
    assert len(p) == len(q) == 64 and p.labels == q.labels == labels
    np.testing.assert_array_equal(p.active, q.active)
    np.testing.assert_array_equal(p.vals, q.vals)  # (NaN where inactive, in both)
    np.testing.assert_array_equal(p.n_active, active.sum(0))
    for r in (0, 17, 63):
        assert p.config(r) == q.config(r) == cfgs[r]
        assert all(type(p.config(r)[lab]) is type(cfgs[r][lab]) for lab in cfgs[r])
    with pytest.raises(ValueError):
        tpe.Pool.from_arrays(d, vals[:, :-1], active[:, :-1])
    bad = active.copy()
    bad[5] = ~bad[5]
    with pytest.raises(ValueError, match="row 5"):
        tpe.Pool.from_arrays(d, vals, bad)


def test_taken_bookkeeping_and_startup_rows():
    d = _domain("quniform_ties")
    p = tpe.Pool(d, [{"q": float(i % 11), "u": i / 50.0} for i in range(50)])
    assert p.n_untaken == 50 and p.taken.dtype == np.uint8 and not p.taken.any()
    p.mark_taken([3, 7, 7])
    p.row_of[100] = 3
    p.row_of[101] = 7
    assert p.n_untaken == 48 and p.taken[[3, 7]].all()
    p.release([3])
    assert p.n_untaken == 49 and not p.taken[3] and p.row_of == {101: 7}
    with pytest.raises(IndexError):
        p.mark_taken([50])
    # the startup rule: a function of (seed, taken set), distinct untaken rows
    a, b = startup_rows(p, 5, 10), startup_rows(p, 5, 10)
    np.testing.assert_array_equal(a, b)
    assert len(set(a.tolist())) == 10 and 7 not in a
    untaken = np.flatnonzero(p.taken == 0)
    np.testing.assert_array_equal(
        a, untaken[np.random.RandomState(5).choice(untaken.size, 10, replace=False)])
    assert sorted(startup_rows(p, 1, 99).tolist()) == untaken.tolist()  # fewer rows than asked
    p.mark_taken(np.arange(50))
    assert startup_rows(p, 1, 4).size == 0
    # no rows left: nothing is scored and no document comes back
    assert tpe.suggest_from_pool([0, 1], d, None, 0, pool=p) == []


def test_pool_entry_points_check_arguments():
    """tpe_pool_fold / tpe_pool_topk report argument errors before any launch
    and return 0 when there is nothing to do (no GPU needed here)."""
    lib = L.load()
    one = ctypes.c_void_p(8)  # a non-null stand-in: validation fails before any launch
    off = np.zeros(2, np.int64)
    col = np.zeros(2, np.int64)
    op, cp = off.ctypes.data, col.ctypes.data

    def fold(n_rows=10, n_labels=2, ld=10, init=1, ptr=one, S=one, terms=None, terms_ld=0):
        return lib.tpe_pool_fold(ptr, ptr, op, cp, n_labels, ptr, ld, n_rows, init, S, terms,
                                 terms_ld, None)
    assert fold(n_rows=0) == 0 and fold(n_rows=0, ptr=None, S=None) == 0  # nothing to do
    assert fold(n_labels=0, init=0, ptr=None, S=None) == 0
    assert fold(n_rows=-1) == -1 and b"tpe_pool_fold" in lib.tpe_last_error()
    assert fold(n_labels=-1) == -1
    assert fold(ptr=None) == -1 and b"null pointer" in lib.tpe_last_error()
    assert fold(S=None) == -1 and b"null pointer" in lib.tpe_last_error()
    assert fold(n_labels=0, init=1, S=None) == -1  # S = 0 still needs S
    assert fold(ld=9) == -1 and b"ld=9" in lib.tpe_last_error()
    assert fold(terms=one, terms_ld=9) == -1 and b"terms_ld=9" in lib.tpe_last_error()
    off[1] = -4
    assert fold() == -1 and b"label 1" in lib.tpe_last_error()
    off[1] = 0

    def topk(n_rows=10, k=3, ptr=one, count=one):
        return lib.tpe_pool_topk(ptr, ptr, n_rows, k, ptr, count, ptr, None)
    assert topk(n_rows=0, ptr=None, count=None) == 0 and topk(k=0, ptr=None, count=None) == 0
    assert topk(n_rows=-1) == -1 and b"n_rows=-1" in lib.tpe_last_error()
    assert topk(k=-2) == -1 and b"k=-2" in lib.tpe_last_error()
    assert topk(ptr=None) == -1 and b"null pointer" in lib.tpe_last_error()
    assert topk(count=None) == -1 and b"null pointer" in lib.tpe_last_error()
    assert lib.tpe_pool_topk_scratch_bytes(-1, 0) == -1
    assert lib.tpe_pool_topk_scratch_bytes(5, -1) == -1
    small, big = lib.tpe_pool_topk_scratch_bytes(100, 5), lib.tpe_pool_topk_scratch_bytes(
        1 << 20, 1 << 30)  # k is clipped to the rows
    assert small >= 16 * 5 and big >= 16 * (1 << 20) + 16 * 256
    assert big == lib.tpe_pool_topk_scratch_bytes(1 << 20, 1 << 20)
