"""The joint scorers against the bits recorded before they shared one walk
kernel, one merge and one host driver (tests/golden/joint_score_bits.npz,
written by tools/record_joint_bits.py): tpe_joint_score, tpe_joint_score_rows
and tpe_joint_chain_rows_keep on the harness of test_gpu_joint_chain_stages.py
(300 pool rows, a 512-trial history, labels of every kind, rows that hold an
option of probability 0) at the pass and chunk edges; the list scorer on the
harness of test_gpu_joint_tree_stages.py; the dense scorer on two cases of
test_gpu_joint_stages.py; and the two other users of the merge, a grid-pool
joint score (test_gpu_grid_joint_stages.py) and a ``loo_label_curves`` curve
(test_gpu_loo_label.py).

The stage tests compare one entry with another (list against dense, one walk
against two calls); they would pass if all entries moved together.  This file
would not.  A NaN (-inf - -inf) is recorded as one fixed pattern: its place is
compared, its own bits are not.
"""
import os

import numpy as np
import pytest

from hyperopt_amd import _lib as L

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "joint_score_bits.npz")
FILL = -1234.5
SIZES = [0, 7, 8, 255, 256, 512]     # n: the pass edge (8 per pass) and the chunk edge (256)
N_CTX = [1, 3, 5]
MODES = [0, L.JOINT_OUT_SCATTER, L.JOINT_OUT_SCATTER | L.JOINT_OUT_ADD]
LIST_BEGIN, MAX_ROWS, LISTED = 100, 128, 137   # the window ends 91 positions past the list
CASES = ["world-%d" % n for n in SIZES] + ["tree-list", "stages", "grid", "loo-label"]


def _bits(a):
    a = np.array(a, np.float64)
    a[np.isnan(a)] = np.nan  # (one pattern for every NaN)
    return np.ascontiguousarray(a).view(np.uint64)


def _list(P, zero_rows):
    """137 distinct rows of a seeded permutation, the zero-probability rows
    inside the window [100, 137)."""
    rows = [r for r in np.random.RandomState(2).permutation(P) if r not in zero_rows][:LISTED - 2]
    rows[LIST_BEGIN + 1:LIST_BEGIN + 1] = zero_rows[:1]
    rows[LIST_BEGIN + 20:LIST_BEGIN + 20] = zero_rows[1:]
    assert len(rows) == LISTED == len(set(rows))
    return np.asarray(rows, np.int64)


def _world(n):
    """Dense, list and chain values on test_gpu_joint_chain_stages.py's world."""
    from tests import test_gpu_joint_chain_stages as S
    w = S._world()
    t, dev = S._torch()
    dj, D, dset = w.dj, len(w.models), w.full_set(n)
    head = (dj.host.ctypes.data, dj.dev.data_ptr(), D)
    mid = (dj.tables.data_ptr(), dj.n_tables, dset.data_ptr(), n, w.vals.data_ptr(), w.ld, w.n_cols)
    got = {}

    def dense(row_begin, n_rows, sub):
        out = t.full((n_rows + S.GUARD,), FILL, dtype=t.float64, device=dev)
        L.check(w.lib.tpe_joint_score(*head, *mid, row_begin, n_rows,
                                      None if sub is None else sub.data_ptr(), out.data_ptr(),
                                      w.scratch.data_ptr(), w.sp), "tpe_joint_score")
        return out.cpu().numpy()

    got["dense"] = dense(0, S.P_ROWS, None)
    assert np.isneginf(got["dense"][S.ZERO_ROWS]).all() and (got["dense"][S.P_ROWS:] == FILL).all()
    sub = S._up(np.random.RandomState(4).normal(size=MAX_ROWS) * 50.0)
    got["dense-sub"] = dense(3, 64, sub)

    rows = S._up(_list(S.P_ROWS, S.ZERO_ROWS))
    count = S._up(np.asarray([LISTED], np.int64))
    tail = (rows.data_ptr(), count.data_ptr(), LIST_BEGIN, MAX_ROWS, sub.data_ptr())
    S0 = np.full(w.ld, 1.5)
    for mode in MODES:
        out = S._up(S0 if mode else np.full(MAX_ROWS, FILL))
        L.check(w.lib.tpe_joint_score_rows(*head, *mid, *tail, out.data_ptr(), mode,
                                           w.scratch.data_ptr(), w.sp), "tpe_joint_score_rows")
        got["list-%d" % mode] = out.cpu().numpy()
    assert (got["list-0"][LISTED - LIST_BEGIN:] == FILL).all()
    for n_ctx in N_CTX:
        for mode in MODES:
            out = S._up(S0 if mode else np.full(MAX_ROWS, FILL))
            keep = [t.full((w.ld,), FILL, dtype=t.float64, device=dev) for _ in range(2)]
            L.check(w.lib.tpe_joint_chain_rows_keep(
                *head, n_ctx, *mid, *tail, out.data_ptr(), mode, keep[0].data_ptr(),
                keep[1].data_ptr(), w.ld, w.scratch.data_ptr(), w.sp), "tpe_joint_chain_rows_keep")
            got["chain-%d-%d" % (n_ctx, mode)] = out.cpu().numpy()
            if not mode:
                got["chain-%d-full" % n_ctx] = keep[0].cpu().numpy()
                got["chain-%d-ctx" % n_ctx] = keep[1].cpu().numpy()
        assert (got["chain-%d-full" % n_ctx] != FILL).sum() == LISTED - LIST_BEGIN
    return got


def _tree_list():
    """tpe_joint_score_rows on test_gpu_joint_tree_stages.py's scorer (sets of
    7 + 1 and 613 + 1 components), the three output modes."""
    from tests import test_gpu_joint_tree_stages as S
    sc = S._scorer()
    rows = _list(sc.P, [5, 299])
    sub = np.random.RandomState(4).normal(size=MAX_ROWS) * 50.0
    got = {}
    for s in (0, 1):
        for mode in MODES:
            out = np.full(sc.ld, 1.5) if mode else np.full(MAX_ROWS, FILL)
            got["%d-%d" % (s, mode)] = sc.call(s, rows, LISTED, LIST_BEGIN, MAX_ROWS, mode, out,
                                               sub=sub)
    return got


def _stages():
    """tpe_joint_score on two cases of test_gpu_joint_stages.py: chunks whose
    every component is dead, and the factor edges of a quantized log label."""
    from tests import test_gpu_joint_stages as S
    got = {}
    for name in ("dead_chunks", "edge_qlognormal"):
        dc = S._dev(name)
        for s in range(len(dc.case["sets"])):
            got["%s-%d" % (name, s)] = dc.log_l(s)
        dset, n, _ = dc.prep(0)
        got[name + "-sub"] = dc.score(dset, n, sub=dc._up(got[name + "-0"]))
    return got


def _grid():
    """tpe_grid_joint_score on test_component_counts' block, one and two chunks."""
    from tests import test_gpu_grid_joint_stages as S
    got = {}
    for n in (8, 257):
        p, block = S._geo("comp", [3, 2, 5, 2, 7], n=n)
        got["%d" % n] = p.grid(block, 0, 420)
    return got


def _loo_label():
    """One ``loo_label_curves`` curve on test_every_kind's 60-trial history."""
    from hyperopt_amd import hp, tpe
    from hyperopt_amd import joint as J
    from hyperopt_amd import pool as pool_mod
    from tests import joint_util as U
    from tests.refine_util import random_case
    from tests.test_gpu_loo import KW
    domain, _trials, hist, _vals = random_case(U.all_kinds_space(hp), 60, 1, 5)
    eng = tpe.engine()
    mult = dict(zip("cdefghij", J.LOO_GRID[np.random.RandomState(7).randint(0, 16, 8)]))
    curve = J.loo_label_curves(eng, domain, hist, pool_mod._seen_rows(eng, hist), 1.0,
                               len(domain.params), None, KW["prior_weight"], 20,
                               KW["cat_smoothing"], False)
    return {label: curve(mult, label) for label in "cf"}


def parts(case):
    """What is recorded of a case: name -> array, the doubles as uint64."""
    if case.startswith("world-"):
        got = _world(int(case[6:]))
    else:
        got = {"tree-list": _tree_list, "stages": _stages, "grid": _grid,
               "loo-label": _loo_label}[case]()
    return {case + "/" + k: _bits(v) for k, v in got.items()}


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {name: z[name] for name in z.files}


@pytest.mark.parametrize("case", CASES)
def test_recorded_bits(golden, case):
    got = parts(case)
    assert sorted(got) == sorted(k for k in golden if k.startswith(case + "/"))
    for name, a in got.items():
        want = golden[name]
        assert a.dtype == want.dtype and a.shape == want.shape, name
        assert (a == want).all(), (name, int((a != want).sum()))
