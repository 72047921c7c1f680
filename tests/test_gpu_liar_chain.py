"""csrc/tpe_joint_lie_chain.hip on the GPU against ``joint.liar_chain_numpy``.  S_0, A, B
are inputs: |S_k - ref| <= 1e-6 sum over the row's live fits of |U_g0| + |U_gk| + |V_g0| +
|V_gk|.  The reference alone shows every pick >= 100 of the largest free row's bound ahead
of its runner-up (``_margins``; the least over the cases below is 4.2e2).
"""
import functools

import numpy as np
import pytest

from hyperopt_amd import Domain, hp, rand, tpe
from hyperopt_amd import _lib as L
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from tests import joint_chain_util as CU
from tests import joint_tree_util as TU
from tests import joint_util as U
from tests import liar_util as LU
from tests.liar_chain_util import chain_case, chain_space

pytestmark = pytest.mark.gpu

SMOOTHING, BW, LIE = 0.5, 0.25, 0.8
KW = dict(lie_weight=LIE, bandwidth=BW, cat_smoothing=SMOOTHING)
SPACES = {"chain": chain_space, "branch": TU.branch_space}  # "branch": every context empty


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(None)
def _case(shape, P):
    """``chain_case`` (branches mixed row by row); 24 free rows, the first and the last
    among them; past P = 8 one free score is NaN, one place of A and one of B -inf."""
    rng = np.random.RandomState(P)
    domain, trials, pool = chain_case(P, P, SPACES[shape])
    G = len(TU.groups_of(domain))
    free = np.unique(np.concatenate([[0, P - 1], rng.permutation(P)[:22]]))
    S0 = rng.normal(0, 1, P)
    S0[free] = 0.5 * rng.permutation(free.size) + rng.uniform(0, 0.1, free.size)
    A, B = rng.uniform(-6, 2, (P, G)), rng.uniform(-6, 2, (P, G))
    gone = np.ones(P, np.uint8)
    gone[free] = 0
    if P > 8:
        S0[free[3]] = np.nan
        A[free[5], 0], B[free[7], 1:] = -np.inf, -np.inf
    return domain, trials, pool, S0, A, B, gone


def _reference(shape, P, k, state=False):
    domain, trials, pool, S0, A, B, gone = _case(shape, P)
    hist = tpe.collect_history(trials, pool.labels)
    return J.liar_chain_numpy(domain, hist, pool.vals, k, pool.active, taken=gone, S0=S0, A=A, B=B,
                              return_state=state, **KW)


def _bound(state):
    U0, Uk, V0, Vk = (np.nan_to_num(np.abs(m), nan=0.0, posinf=0.0) for m in state)
    return 1e-6 * (U0 + Uk + V0 + Vk).sum(1)


def _margins(shape, P):
    """Per pick: its gap to the runner-up over the largest bound of a free row (NaN picks out)."""
    pool, gone = _case(shape, P)[2], _case(shape, P)[6].astype(bool).copy()
    X = [list(v) for v in pool.vals]
    out = []
    for j, p in enumerate(_reference(shape, P, P + 2)[0]):
        ref = _reference(shape, P, j, state=True)
        gap = LU.gap_to_runner_up(ref[2], gone, int(p), X)
        out.append(gap / max(_bound(ref[3:])[~gone].max(), 1e-300))
        gone[p] = True
    return np.asarray([m for m in out if m == m])


def _device(shape, P, k, rows=None, tree=False):
    import torch as t
    domain, trials, pool, S0, A, B, gone = _case(shape, P)
    sel = np.arange(P) if rows is None else rows
    eng = tpe.engine()
    d = tpe.Pool.from_arrays(domain, pool.vals[sel], pool.active[sel]).device(eng)
    fits = pool_mod._fit(eng, domain, tpe.collect_history(trials, pool.labels), len(pool.labels),
                         pool_mod._settings(1.0, 0.25, 25, "tree" if tree else "chain", BW,
                                            SMOOTHING))
    up = lambda a: t.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    odd = (np.arange(P) % 2).astype(np.uint8)
    head = (fits, d.vals, d.active, d.vals.shape[1], d.vals.shape[0], sel.size, up(S0[sel]))
    tail = (up((gone * odd)[sel]), up((gone * (1 - odd))[sel]), k, LIE, True)
    if tree:
        return J.liar_tree_device(*head, up(A[sel].T), *tail)
    return J.liar_chain_device(*head, up(A[sel].T), up(B[sel].T), *tail)


@pytest.mark.parametrize("P", [1, 256, 257, 600])
def test_picks_and_scores_match_the_numpy_definition(P):
    S0, gone = _case("chain", P)[3], _case("chain", P)[6]
    margins = _margins("chain", P)
    print("P=%d least margin %.3g" % (P, min(margins, default=np.inf)))
    assert (margins >= 100.0).all()  # (the reference's own: the inputs' property)
    for k in (1, 3, P + 2):
        ref = _reference("chain", P, k, state=True)
        rows, at, S_k = _device("chain", P, k)
        assert rows.tolist() == ref[0].tolist() and len(rows) == min(k, int((gone == 0).sum()))
        bound = _bound(ref[3:])
        for got, want, b in ((S_k, ref[2], bound), (at, ref[1], bound[rows])):
            np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
            ok = ~np.isnan(want)
            assert (np.abs(got[ok] - want[ok]) <= b[ok]).all()
        assert (_bits(at[:1]) == _bits(S0[rows[:1]])).all()  # k = 1: the plain first row


@pytest.mark.parametrize("P,k", [(1, 1), (257, 3), (600, 602)])
def test_empty_contexts_have_the_bits_of_the_tree_call(P, k):
    chain, tree = _device("branch", P, k), _device("branch", P, k, tree=True)
    assert chain[0].tolist() == tree[0].tolist() and len(chain[0]) in (k, 23, 24)
    assert (_bits(chain[1]) == _bits(tree[1])).all() and (_bits(chain[2]) == _bits(tree[2])).all()


def test_bits_do_not_depend_on_the_pool_shape():
    rows, at, S_k = _device("chain", 600, 6)
    rest = np.setdiff1d(np.arange(600), rows)
    sub = np.sort(np.concatenate([rows, np.random.RandomState(9).permutation(rest)[:251]]))
    rows2, at2, S_k2 = _device("chain", 600, 6, rows=sub)
    assert sub.size == 257 and sub[rows2].tolist() == rows.tolist()
    assert (_bits(S_k2) == _bits(S_k[sub])).all() and (_bits(at2) == _bits(at)).all()


@pytest.mark.parametrize("n", [0, 255, 256])
def test_score_tree_device_keeps_both_above_values(n):
    """Group ``b`` of ``cross_space`` (context ``a``): n above trials, n + 1 components."""
    import torch as t
    rng = np.random.RandomState(n)
    domain = Domain(lambda x: 0, CU.cross_space())
    cfgs = [{"a": int(rng.randint(4)), "v": 1, "c": float(rng.uniform())} for _ in range(30)]
    cfgs += [{"a": int(rng.randint(4)), "v": 0, "b": int(rng.randint(4))} for _ in range(n)]
    trials = U.make_trials(domain, cfgs, [0.01 * i for i in range(len(cfgs))])  # below: branch 1
    pool = tpe.Pool(domain, [rand.sample_config(domain, rng) for _ in range(40)])
    P = len(pool)
    S = tpe.score_configs(domain, trials, pool, joint="chain")
    st = pool_mod._settings(1.0, 0.25, 25, "chain", batch="liar-chain")
    eng, d = pool_mod._score_device(domain, trials, pool, st, False)
    ref = CU.chain_reference(domain, trials, pool.vals, pool.active)
    assert (_bits(d.S[:P].cpu().numpy()) == _bits(S)).all() and ref[6][1][1] == n
    for kept, want in ((d.above, ref[3]), (d.above_ctx, ref[5])):
        got, live = kept.cpu().numpy().T[:P], ~np.isnan(want)
        assert live[:, 1:].any() and np.allclose(got[live], want[live], rtol=1e-6, atol=0.0)
    # the subtrahend of group 1 by itself: tpe_joint_chain_rows, dense, no sub
    f, lib = d.fits[1], L.load()
    rows = t.from_numpy(np.flatnonzero(~np.isnan(ref[3][:, 1]))).to(eng.device)
    count, dense = t.tensor([len(rows)], device=eng.device), t.empty_like(d.above[1][:len(rows)])
    scratch = dense.new_empty(lib.tpe_joint_chain_scratch_bytes(P, n) + 16, dtype=t.uint8)
    L.check(lib.tpe_joint_chain_rows(
        f.dj.host.ctypes.data, f.dj.dev.data_ptr(), len(f.dj.models), f.n_ctx,
        f.dj.tables.data_ptr(), f.dj.n_tables, f.sets[1][0].data_ptr(), n, d.vals.data_ptr(),
        d.vals.shape[1], d.vals.shape[0], rows.data_ptr(), count.data_ptr(), 0, rows.numel(), None,
        dense.data_ptr(), 0, scratch.data_ptr(), f.sp), "tpe_joint_chain_rows")
    assert rows.numel() and (_bits((d.above[1] - d.above_ctx[1])[rows].cpu().numpy()) ==
                             _bits(dense.cpu().numpy())).all()


def test_public_path_on_a_quantized_chain_space():
    """Good trials at one (root, branch 0) point; the pool: both branches' 16 x 16 lattices."""
    lat = lambda name: hp.quniform(name, 0, 15, 1)  # noqa: E731
    space = {"x": lat("x"), "v": hp.choice("v", [{"y": lat("y")}, {"c": lat("c")}])}
    domain, rng, at = Domain(lambda x: 0, space), np.random.RandomState(2), range(16)
    cfgs = [{"x": 6.0, "v": 0, "y": 10.0}] * 10
    cfgs += [{"x": float(a), "v": 0, "y": float(b)} for a, b in rng.randint(0, 16, (20, 2))]
    cfgs += [{"x": float(a), "v": 1, "c": float(c)} for a, c in rng.randint(0, 16, (10, 2))]
    trials = U.make_trials(domain, cfgs, [0.01 * i + (i >= 10) for i in range(40)])
    pool = tpe.Pool(domain, [{"x": float(x), "v": 0, "y": float(y)} for x in at for y in at] +
                    [{"x": float(x), "v": 1, "c": float(c)} for x in at for c in at])
    hist = tpe.collect_history(trials, pool.labels)
    kw = dict(gamma=1.5)  # ceil(1.5 sqrt(40)) = 10 below rows: the good trials
    ref_rows = J.liar_chain_numpy(domain, hist, pool.vals, 8, pool.active, **kw)[0]
    S0 = J.score_numpy(domain, hist, pool.vals, pool.active, tree="chain", **kw)
    top, v = np.argsort(-S0, kind="stable")[:8], np.nan_to_num(pool.vals)
    spread = lambda r: np.linalg.norm(v[r][:, None] - v[r][None], axis=2).sum() / 56  # noqa: E731
    assert ref_rows[0] == top[0] and spread(ref_rows) > spread(top)
    rows = tpe.pick_batch(domain, trials, pool, 8, joint="chain", batch="liar-chain", **kw)
    assert rows.tolist() == ref_rows.tolist()
    # a sampled pool, either draw: k distinct documents, in the startup phase too
    skw = dict(n_EI_candidates=512, joint="chain", batch="liar-chain", verbose=False)
    for more in (dict(draw="joint"), dict(), dict(n_startup_jobs=10 ** 6)):
        docs = tpe.suggest_sampled(list(range(500, 506)), domain, trials, 21, distinct=True,
                                   **skw, **more)
        assert len({str(sorted(d["misc"]["vals"].items())) for d in docs}) == 6 == len(docs)
