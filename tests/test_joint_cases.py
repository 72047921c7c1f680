"""The premises of tests/test_gpu_joint_stages.py, checked without a GPU.

The GPU tests hold the joint kernels to K * 2**-53 * cond against the 50-digit
values of tests/golden/joint_cases.npz.  Here: that the fixture is the case
table's, that the two fp64 forms of the definition (tests/joint_util.py's scalar
functions, joint.score_numpy's numpy) meet it within K_CPU -- where K_CPU is
measured -- that every row is well conditioned, and that each case has the
property it is named for.
"""
import importlib.util
import os

import numpy as np
import pytest

from hyperopt_amd import joint as J
from hyperopt_amd import tpe
from tests import joint_cases as JC

_A = {}


def _a(name, s=0):
    """The fp64 scalar restatement's (P, C) a_i, computed once per case and set."""
    if (name, s) not in _A:
        _A[name, s] = JC.scalar_a(JC.load()[name], s)
    return _A[name, s]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and (a.view(np.uint64) == b.view(np.uint64)).all()


def test_fixture_holds_the_case_table_inputs():
    cases, built = JC.load(), JC.build_inputs()
    assert set(cases) == set(built) | {"all_kinds"}
    for name, b in built.items():
        c = cases[name]
        for k in JC.SCALARS:
            assert c[k] == b[k], (name, k)
        for k in JC.INPUT_KEYS:
            if k not in b:
                assert k not in c
            elif k == "sets":
                assert len(c[k]) == len(b[k])
                assert all(np.array_equal(x, y) and x.dtype == y.dtype
                           for x, y in zip(c[k], b[k])), name
            elif k == "labels":
                assert c[k].tobytes() == b[k].tobytes() and c[k].dtype == b[k].dtype, name
            else:
                assert c[k].dtype == b[k].dtype and c[k].tobytes() == b[k].tobytes(), (name, k)
    assert os.path.getsize(JC.FIXTURE) < 300 * 1024


def test_case_table_has_the_geometry_it_names():
    cases = JC.load()
    chunk = 256
    assert [cases["geo%d" % C]["sets"][0].size + 1 for C in JC.GEO_C] == list(JC.GEO_C)
    assert {(C - 1) % 8 for C in JC.GEO_C} == set(range(8))      # the prior's place in its pass
    assert {C % chunk for C in JC.GEO_C} >= {0, 1}
    for C in JC.ONEHOT_C:
        want = {0, 7, 8, C - 2, C - 1} | {i for i in (255, 256, 257) if i < C}
        assert set(cases["geo%d" % C]["onehot"].tolist()) == want
    for name in ("run_up", "run_down", "run_mid", "dead_chunks", "dead_passes"):
        assert cases[name]["sets"][0].size == 512 and len(cases[name]["labels"]) == 1
    for D in JC.LABEL_COUNTS:
        c = cases["labels%d" % D]
        cols = c["labels"]["col"]
        assert len(cols) == D and len(set(cols.tolist())) == D and c["pool"].shape[1] > D
        assert not np.array_equal(cols, np.sort(cols)) or D == 1
        unused = np.setdiff1d(np.arange(c["pool"].shape[1]), cols)
        assert np.isnan(c["pool"][:, unused]).all() and np.isnan(c["hist"][:, unused]).all()
        assert np.isfinite(c["pool"][:, cols]).all() and np.isfinite(c["hist"][:, cols]).all()
    prep = cases["prep"]
    assert [s.size for s in prep["sets"]] == list(JC.PREP_N)
    lab = prep["labels"]
    assert 12 in lab["shift"].tolist()
    logs = [d for d in range(len(lab)) if lab["flags"][d] & 1 and not lab["flags"][d] & 2]
    seen = np.concatenate([prep["hist"][prep["sets"][-1]][:, lab["col"][d]] for d in logs])
    assert (seen == 0.0).any() and (seen == 1e-13).any()


def test_fixture_within_k_cpu_of_both_fp64_forms_and_well_conditioned():
    """K_cpu: glibc's libm against the 50-digit values, no code under test."""
    k_numpy, k_scalar, worst = 0.0, 0.0, None
    for name, c in JC.load().items():
        for s in range(len(c["sets"])):
            ref, cond = c["logl"][s], c["cond"][s]
            assert ref.shape == cond.shape == (JC.P,)
            assert (cond >= 1.0).all() and (cond <= 1e6).all(), (name, s, cond.max())
            assert not np.isnan(ref).any() and not np.isposinf(ref).any()
            k = JC.k_of(JC.numpy_log_l(c, s), ref, cond)
            if k > k_numpy:
                k_numpy, worst = k, (name, s)
            k_scalar = max(k_scalar, JC.k_of(JC.scalar_log_l(_a(name, s)), ref, cond))
            np.testing.assert_array_equal(c["sig"][s], JC.bandwidths(c["labels"], c["sets"][s].size,
                                                                     c["bandwidth"]))
            models = JC.models_of(c)
            assert _same_bits(c["sig"][s], J.bandwidths(models, c["sets"][s].size, c["bandwidth"]))
    print("K_cpu: score_numpy %.3g (at %s), scalar restatement %.3g; recorded %g"
          % (k_numpy, worst, k_scalar, JC.K_CPU))
    assert JC.K_CPU / 2 < k_numpy <= JC.K_CPU
    assert k_scalar <= JC.K_CPU
    assert JC.K_DEV == 2.0 ** np.ceil(np.log2(8 * JC.K_CPU))


def test_one_hot_entries_match_the_scalar_restatement():
    for C in JC.ONEHOT_C:
        c = JC.load()["geo%d" % C]
        n = C - 1
        a = _a(c["name"]) - J.log_weights(n, c["lf"], c["prior_weight"])[None, :]
        assert c["onehot_a"].shape == (len(c["onehot"]), JC.P)
        assert np.isfinite(c["onehot_a"]).all()
        assert (c["onehot_cond"] <= 1e6).all()
        for j, i in enumerate(c["onehot"]):
            # (a - log w + log w is not a: one more rounding than K_CPU counts)
            assert JC.k_of(a[:, i], c["onehot_a"][j], c["onehot_cond"][j]) <= JC.K_CPU + 2


def test_fixture_sample_rederived_with_mpmath():
    pytest.importorskip("mpmath")
    path = os.path.join(os.path.dirname(JC.FIXTURE), "make_joint_cases.py")
    spec = importlib.util.spec_from_file_location("make_joint_cases", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    cases = JC.load()
    for name in ("geo9", "edge_quniform", "edge_pchoice", "labels1"):
        c = cases[name]
        for s in range(len(c["sets"])):
            ll, cd, oa, oc = gen.score_set(c, s, onehot=[int(i) for i in c["onehot"]] if s == 0
                                           else ())
            assert _same_bits(ll, c["logl"][s]) and _same_bits(cd, c["cond"][s]), name
            if s == 0 and len(c["onehot"]):
                assert _same_bits(oa, c["onehot_a"]) and _same_bits(oc, c["onehot_cond"])
    for name, rows in (("geo257", [0, 39]), ("dead_chunks", [0, 15, 30]), ("all_kinds", [0, 39])):
        c = cases[name]
        ll, cd = gen.score_set(c, 0, rows=rows)[:2]
        assert _same_bits(ll, c["logl"][0][rows]) and _same_bits(cd, c["cond"][0][rows]), name
    prep = cases["prep"]
    mu, cst, cc = gen.prep_expected(prep, 1)
    assert _same_bits(mu, prep["prep_mu"][1]) and _same_bits(cst, prep["prep_cst"][1])
    assert np.array_equal(cc, prep["prep_cond"][1])


@pytest.mark.parametrize("C", JC.GEO_C)
def test_every_geometry_component_carries_some_row(C):
    """p_i(row) >= 2**-30 for some row: a dropped or mis-scored single component
    moves that row by 2**-30 relative, far beyond K 2**-53 cond."""
    c = JC.load()["geo%d" % C]
    ref = c["logl"][0]
    assert np.isfinite(ref).all()
    p = np.exp(_a(c["name"]) - ref[:, None])
    assert p.shape == (JC.P, C)
    assert (p.max(0) >= 2.0 ** -30).all(), p.max(0).min()
    assert (2.0 ** -30 > 64 * JC.K_DEV * JC.U53 * c["cond"][0]).all()


def test_dead_cases_have_the_pattern_they_claim():
    far, near, out = slice(0, 15), slice(15, 30), slice(30, 40)
    c = JC.load()["dead_chunks"]
    a, ref = _a("dead_chunks"), c["logl"][0]
    assert np.isneginf(a[far, :256]).all() and np.isfinite(a[far, 256:512]).all()
    assert np.isneginf(a[far, 512]).all()           # the prior, alone in chunk 2
    assert np.isfinite(a[near, :256]).all() and np.isneginf(a[near, 256:512]).all()
    assert np.isfinite(a[near, 512]).all()
    assert np.isneginf(a[out]).all()
    assert np.isfinite(ref[:30]).all() and np.isneginf(ref[out]).all()
    c = JC.load()["dead_passes"]
    a, ref = _a("dead_passes"), c["logl"][0]
    even = (np.arange(512) // 64) % 2 == 0
    an, af = a[near][:, :512], a[far][:, :512]
    assert np.isneginf(an[:, even]).all() and np.isfinite(an[:, ~even]).all()
    assert np.isfinite(af[:, even]).all() and np.isneginf(af[:, ~even]).all()
    assert np.isfinite(ref[:30]).all() and np.isneginf(ref[out]).all()


def test_edge_cases_have_the_pattern_they_claim():
    cases = JC.load()

    def pattern(name):
        c = cases[name]
        return c, np.isneginf(c["logl"][0]), np.isneginf(c["logl"][1])

    c, b, a = pattern("edge_qlognormal")
    x = c["pool"][:, 1]
    assert (x == 0.0).sum() > 2 and (x == 1.0).sum() > 2            # x = 0, x = q
    np.testing.assert_array_equal(np.flatnonzero(b), [5])
    np.testing.assert_array_equal(np.flatnonzero(a), [5])
    assert (c["hist"][c["sets"][1], 1] == 0.0).any()
    c, b, a = pattern("edge_qloguniform")
    x = c["pool"][:, 1]
    np.testing.assert_array_equal(b, x == 0.0)
    np.testing.assert_array_equal(a, x == 0.0)
    assert (x == 0.0).sum() > 2 and (x == 20.0).sum() > 2
    c, b, a = pattern("edge_quniform")
    x = c["pool"][:, 1]
    np.testing.assert_array_equal(b, x == -1.5)                      # the upper edge on lo
    np.testing.assert_array_equal(a, x == -1.5)
    assert (x == -1.5).sum() == 2 and (x == 0.0).sum() > 2 and (x == 9.0).sum() > 2
    c, b, a = pattern("edge_lognormal")
    assert (c["pool"][:, 0] == 0.0).sum() == 2 and not b.any() and not a.any()
    c, b, a = pattern("edge_pchoice")
    zero = c["pool"][:, 2] == 0.0
    assert zero.sum() == 3 and JC.label_probs(c, 2)[0] == 0.0
    assert (c["hist"][c["sets"][0], 2] == 0.0).sum() == 1
    assert not (c["hist"][c["sets"][1], 2] == 0.0).any()
    assert not b.any()                        # the component of that category hits
    np.testing.assert_array_equal(a, zero)    # no such component: -inf


@pytest.mark.parametrize("name", ["run_up", "run_down", "run_mid"])
def test_running_maximum_cases_are_monotone_as_named(name):
    a = _a(name)
    assert a.shape == (JC.P, 513) and np.isfinite(a).all()
    assert (a.max(1) - a.min(1) > 800.0).all()
    pm = np.stack([a[:, i0:i0 + 8].max(1) for i0 in range(0, 513, 8)], 1)  # (P, 65 passes)
    assert pm.shape == (JC.P, 65)
    if name == "run_up":        # every pass rescales, the prior's own included
        assert (np.diff(pm, axis=1) > 1e-6).all()
    elif name == "run_down":    # none after the first
        assert (pm[:, 1:] < pm[:, :1] - 1e-6).all()
    else:                       # rises into the middle chunk, never after
        top = pm.argmax(1)
        assert ((top >= 32) & (top < 64)).all() and len(set(top.tolist())) == 1
        t = int(top[0])
        assert (np.diff(pm[:, :t + 1], axis=1) > 1e-6).all()
        assert (pm[:, t + 1:] < pm[:, t:t + 1]).all()


@pytest.mark.parametrize("name", sorted(JC.PUBLIC))
def test_public_cases_are_what_the_package_builds(name):
    """The split of the real Trials gives the fixture's sets, the Domain its
    label records."""
    c = JC.load()[name]
    domain, trials, rows, kw = JC.public_problem(c)
    hist = tpe.collect_history(trials, list(domain.params))
    models = J.label_models(domain)
    cols = [m.col for m in models]
    assert cols == c["labels"]["col"].tolist() == [0, 1, 2]
    np.testing.assert_array_equal(np.asarray(hist.vals)[:, cols], c["hist"])
    isb, isa = tpe.split_masks(hist, kw["gamma"])
    for s, mask in enumerate((isb, isa)):
        np.testing.assert_array_equal(J.set_rows(hist, mask, cols), c["sets"][s])
    assert c["sets"][1].size + 1 == int(name[3:])
    for m, r, want in zip(models, c["labels"], JC.models_of(c)):
        for k in ("kind", "is_log", "bounded", "lo", "hi", "q", "mu", "sigma", "n_cat", "offset"):
            assert getattr(m, k) == getattr(want, k), k
        if m.p is not None:
            np.testing.assert_array_equal(m.p, want.p)
    pool = tpe.Pool(domain, rows)
    np.testing.assert_array_equal(pool.vals, c["pool"])
    hist_j = J.score_numpy(domain, hist, pool.vals, return_parts=True, **kw)
    for s in (0, 1):
        assert JC.k_of(hist_j[1 + s], c["logl"][s], c["cond"][s]) <= JC.K_CPU
