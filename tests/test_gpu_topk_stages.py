"""tpe_pool_topk stage by stage (csrc/tpe_pool.hip): what the six kernels leave
in the caller's scratch -- the radix select's control block and bins, the tile
table after the scan, the candidate list before the rank -- against the numpy
replay of tests/topk_cases.py, and the final rows against the lexsort rule
(test_gpu_pool._expected_order), on the cases of that file: one deciding
radix pass at a time, k inside a tie class spread over the tiles, winners at
thread and tile edges, k around the rank's LDS tiles, 258 and 514 tiles (the
scan's threads own several), nothing untaken.  Everything is compared exactly;
the scratch is laid out by tpe_pool_topk_layout, not by constants here.

Then the scratch as pool._topk_device keeps it (one buffer, grown and reused
across calls), and suggest_from_pool over a GridPool of 261 tiles.
"""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import Domain, Trials, fmin, hp, rand, tpe
from hyperopt_amd import _lib as L
from hyperopt_amd import pool as pool_mod
from tests import topk_cases as TC
from tests.test_gpu_pool import _expected_order

pytestmark = pytest.mark.gpu

GUARD = 64      # bytes after the scratch that must stay as they were
POISON = -7


class _TopK(object):
    """tpe_pool_topk through the C ABI on one (S, taken), uploaded once (or
    device tensors already)."""

    def __init__(self, S, taken):
        import torch
        self.t, self.lib = torch, L.load()
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.n = len(S)
        if not torch.is_tensor(S):
            # (copies: a case's arrays are read-only)
            S = torch.from_numpy(np.array(S, np.float64)).to(self.dev)
            taken = torch.from_numpy(np.array(taken, np.uint8)).to(self.dev)
        self.S, self.taken = S, taken

    def layout(self, k):
        out = (ctypes.c_int64 * 7)()
        assert self.lib.tpe_pool_topk_layout(self.n, k, ctypes.cast(out, ctypes.c_void_p), 7) == 7
        return list(out)

    def fresh(self, k):
        total = self.layout(k)[5]
        return self.t.full((total + GUARD,), 0xFF, dtype=self.t.uint8, device=self.dev)

    def __call__(self, k, ws):
        """(out_rows with one guard word on either side, count)."""
        t = self.t
        slots = max(min(k, self.n), 1)
        out = t.full((slots + 2,), POISON, dtype=t.int64, device=self.dev)
        cnt = t.full((1,), POISON, dtype=t.int64, device=self.dev)
        sp = ctypes.c_void_p(t.cuda.current_stream(self.dev).cuda_stream)
        L.check(self.lib.tpe_pool_topk(self.S.data_ptr(), self.taken.data_ptr(), self.n, k,
                                       out.data_ptr() + 8, cnt.data_ptr(), ws.data_ptr(), sp),
                "tpe_pool_topk")
        t.cuda.synchronize(self.dev)
        return out.cpu().numpy(), int(cnt.item())


def _check_scratch(raw, lay, n, k, r):
    """The scratch bytes ``raw`` of a call that started from 0xFF bytes."""
    ctl, bins, tile, ckey, crow, total, per_tile = lay
    assert per_tile == TC.TILE
    words = raw[ctl:ctl + 40].copy()
    prefix, mask = (int(v) for v in words[:16].view(np.uint64))
    k_rem, k_eff, n_less = (int(v) for v in words[16:].view(np.int64))
    print("T=%016x mask=%016x k_rem=%d k_eff=%d n_less=%d" % (prefix, mask, k_rem, k_eff, n_less))
    # -- the control block
    assert (k_rem, k_eff, n_less) == (r.k_rem, r.k_eff, r.n_less)
    assert prefix == int(r.T) and mask == int(r.mask)
    if k_eff > 0:
        assert mask == (1 << 64) - 1
    # -- the bins are zero after the last pass
    assert not raw[bins:bins + 8 * 256].any()
    # -- the tile table: exclusive offsets, both columns, every tile
    n_tiles = (n + per_tile - 1) // per_tile
    got = raw[tile:tile + 16 * n_tiles].copy().view(np.int64).reshape(n_tiles, 2)
    np.testing.assert_array_equal(got, r.tile_off)
    # -- the candidate list, in the replay's order; nothing past k_eff
    slots = min(k, n)
    got_key = raw[ckey:ckey + 8 * k_eff].copy().view(np.uint64)
    got_row = raw[crow:crow + 8 * k_eff].copy().view(np.int64)
    np.testing.assert_array_equal(got_row, r.cand_row)
    np.testing.assert_array_equal(got_key, r.cand_key)
    assert (raw[ckey + 8 * k_eff:ckey + 8 * slots] == 0xFF).all()
    assert (raw[crow + 8 * k_eff:crow + 8 * slots] == 0xFF).all()
    # -- and nothing past the scratch
    assert raw.size == total + GUARD and (raw[total:] == 0xFF).all()


@pytest.mark.parametrize("name", TC.NAMES)
def test_stages(name):
    c = TC.case(name)
    n, k = c.S.size, c.k
    r = TC.replay(c.S, c.taken, k)
    want = _expected_order(c.S, c.taken, k)
    run = _TopK(c.S, c.taken)
    lay = run.layout(k)
    assert lay[5] == run.lib.tpe_pool_topk_scratch_bytes(n, k)
    ws = run.fresh(k)
    out, count = run(k, ws)
    raw = ws.cpu().numpy()
    _check_scratch(raw, lay, n, k, r)
    # -- the output: the rule's rows, their number, nothing else written
    assert count == r.k_eff == want.size
    np.testing.assert_array_equal(out[1:1 + count], want)
    assert (out[1 + count:] == POISON).all() and out[0] == POISON
    # -- again into the scratch this call left behind
    out2, count2 = run(k, ws)
    assert count2 == count and out2.tobytes() == out.tobytes()
    assert ws.cpu().numpy().tobytes() == raw.tobytes()
    # -- and into a scratch that a larger (n, k) has just used
    t = run.t
    gen = t.Generator(device=run.dev)
    gen.manual_seed(n + k)
    n2, k2 = n + TC.TILE + 3, k + 300
    big = _TopK(t.round(t.randn(n2, dtype=t.float64, device=run.dev, generator=gen), decimals=1),
                t.zeros(n2, dtype=t.uint8, device=run.dev))
    ws2 = big.fresh(k2)
    assert ws2.numel() > ws.numel()
    _, count_big = big(k2, ws2)
    assert count_big == k2
    out3, count3 = run(k, ws2)
    assert count3 == count and out3.tobytes() == out.tobytes()


def test_topk_device_grows_and_reuses_its_buffers():
    """pool._topk_device keeps one scratch, one row buffer and one count per
    pool and grows them: k = 3, 64, 5, 64 on one pool, scores full of ties."""
    import torch
    domain = Domain(lambda p: 0.0, {"x": hp.uniform("x", 0, 1)})
    P = TC.N3
    rng = np.random.RandomState(77)
    pool = tpe.Pool.from_arrays(domain, rng.uniform(size=(P, 1)), np.ones((P, 1), bool))
    pool.mark_taken(np.flatnonzero(rng.uniform(size=P) < 0.3))
    S = np.round(rng.normal(size=P), 1)
    S[rng.permutation(P)[:4]] = [np.nan, np.inf, -0.0, 0.0]
    eng = tpe.engine()
    d = pool_mod._mirror(pool, eng)
    d.S[:P].copy_(torch.from_numpy(S))
    sizes = []
    for k in (3, 64, 5, 64):
        rows = pool_mod._topk_device(eng, d, P, k)
        np.testing.assert_array_equal(rows, _expected_order(S, pool.taken, k), err_msg="k=%d" % k)
        sizes.append((d.scratch.numel(), d.rows_out.numel(), d.scratch.data_ptr()))
    assert sizes[0][0] < sizes[1][0] and sizes[0][1] == 3 and sizes[1][1] == 64
    assert sizes[1] == sizes[2] == sizes[3]   # (kept, not allocated again)


def test_suggest_from_a_grid_pool_beyond_256_tiles():
    """suggest_from_pool over 129 x 129 x 64 = 1 065 024 rows (261 tiles: a
    scan thread owns two), the best rows excluded: the rule's rows of the
    pool's own scores."""
    space = {"a": hp.uniform("a", 0, 1), "b": hp.normal("b", 0, 2), "c": hp.loguniform("c", -3, 0)}
    trials = Trials()
    fmin(lambda p: (p["a"] - 0.3) ** 2 + 0.1 * (p["b"] - 1.0) ** 2 + p["c"], space,
         algo=rand.suggest, max_evals=40, trials=trials, rstate=np.random.RandomState(5),
         show_progressbar=False)
    domain = Domain(lambda p: 0.0, space)
    grid = tpe.GridPool(domain, {"a": np.linspace(0.0, 1.0, 129), "b": np.linspace(-4.0, 4.0, 129),
                                 "c": np.exp(np.linspace(-2.9, -0.1, 64))})
    P = len(grid)
    assert P == 129 * 129 * 64 and (P + TC.TILE - 1) // TC.TILE > 257
    assert TC.scan_owner((P + TC.TILE - 1) // TC.TILE)[0] == 2
    S = tpe.score_configs(domain, trials, grid)
    assert S.shape == (P,) and np.isfinite(S).all()
    order = _expected_order(S, np.zeros(P, np.uint8), 40)
    rng = np.random.RandomState(6)
    grid.exclude(np.concatenate([order[[0, 1, 3, 7]], rng.permutation(P)[:1000]]))
    want = _expected_order(S, grid.excluded, 8)
    assert not set(want.tolist()) & set(order[[0, 1, 3, 7]].tolist())
    ids = trials.new_trial_ids(8)
    docs = tpe.suggest_from_pool(ids, domain, trials, 1, pool=grid, verbose=False)
    assert [grid.row_of[d["tid"]] for d in docs] == want.tolist()
