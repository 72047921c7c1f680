"""The top-k cases (tests/topk_cases.py) are what they are named for, and the
numpy replay of tpe_pool_topk's stages ends in the order of the lexsort rule
(test_gpu_pool._expected_order), which stays the reference of the final order.
Building a case runs its builder's own assertions: the digit a pass decides
on, the tie class that k cuts, which k_pool_scan thread owns which tile.
tpe_pool_topk_layout is host code and is checked here too.
tests/test_gpu_topk_stages.py runs the kernels on the same table.
"""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _lib as L
from tests import topk_cases as TC
from tests.test_gpu_pool import TILE, _expected_order


def test_case_table():
    assert len(set(TC.NAMES)) == len(TC.NAMES) and TC.TILE == TILE
    for p in range(8):
        for k in (1, 100, 257, 5000):
            assert "digit-%d-k%d" % (p, k) in TC.NAMES
    for k in (255, 256, 257, 512, 513):
        assert "rank-k%d" % k in TC.NAMES
    for kind, hi in (("plain", "hi"), ("plain", "nohi"), ("zero", "hi"), ("zero", "nohi"),
                     ("nan", "nohi")):
        for cut in ("1", "2", "tile0", "tile0+1", "all-1", "all"):
            assert "ties-%s-%s-%s" % (kind, hi, cut) in TC.NAMES
    for n in (1, 16, 17, 4096, 4097):
        assert "edges-n%d-w0" % n in TC.NAMES
    for name in ("tiles-257", "tiles-514"):
        for variant in ("spread", "cross"):
            for k in (1, 64, 1000):
                assert "%s-%s-k%d" % (name, variant, k) in TC.NAMES
    assert {"staircase", "none-free", "k-over-free+7", "k-over-n+5"} <= set(TC.NAMES)
    assert TC.BIG == {"tiles-257": 257 * 4096 + 1, "tiles-514": 513 * 4096 + 5}
    # k_pool_scan's split (one block of 256 threads): per = 1 up to 256 tiles
    assert TC.scan_owner(4) == (1, 4, 1) and TC.scan_owner(256) == (1, 256, 1)
    assert TC.scan_owner(258) == (2, 129, 2) and TC.scan_owner(514) == (3, 172, 1)


def test_pool_key():
    s = np.array([np.nan, -np.nan, np.inf, 1.0, 0.0, -0.0, -1.0, -np.inf])
    key = TC.pool_key(s)
    assert key[0] == key[1] == 1 and key[4] == key[5]
    assert (np.diff(key[[1, 2, 3, 4, 6, 7]].astype(object)) > 0).all()
    finite = s[2:]
    back = TC.from_keys(TC.pool_key(finite))
    assert np.array_equal(back == 0.0, finite == 0.0) and np.array_equal(back[back != 0.0],
                                                                         finite[finite != 0.0])


@pytest.mark.parametrize("name", TC.NAMES)
def test_replay_is_the_rule(name):
    c = TC.case(name)   # (the builder's assertions run here)
    n = c.S.size
    assert c.taken.shape == (n,) and set(np.unique(c.taken).tolist()) <= {0, 1}
    r = TC.replay(c.S, c.taken, c.k)
    free = int((c.taken == 0).sum())
    assert r.k_eff == min(c.k, free) <= 5000
    np.testing.assert_array_equal(r.out, _expected_order(c.S, c.taken, c.k))
    # the replay with itself: the list is the selected rows once each, the last
    # tile's offsets and counts add up to n_less and the tie class
    assert r.cand_row.size == r.cand_key.size == r.k_eff == r.n_less + r.k_rem
    assert np.unique(r.cand_row).size == r.k_eff and not c.taken[r.cand_row].any()
    assert r.tile_off.shape == ((n + TILE - 1) // TILE, 2) and (r.tile_off[0] == 0).all()
    assert (np.diff(r.tile_off, axis=0) >= 0).all()
    if r.k_eff:
        assert (r.cand_key[:r.n_less] < r.T).all() and (r.cand_key[r.n_less:] == r.T).all()
        assert (np.diff(r.cand_row[:r.n_less]) > 0).all()
        assert (np.diff(r.cand_row[r.n_less:]) > 0).all()
        last = np.arange(n) >= (r.tile_off.shape[0] - 1) * TILE
        fk = (c.taken == 0) & last
        assert r.tile_off[-1, 0] + int((fk & (r.keys < r.T)).sum()) == r.n_less
        assert r.tile_off[-1, 1] + int((fk & (r.keys == r.T)).sum()) >= r.k_rem


def _layout(lib, n_rows, k, n=7):
    out = (ctypes.c_int64 * 8)(*([-7] * 8))
    rc = lib.tpe_pool_topk_layout(n_rows, k, ctypes.cast(out, ctypes.c_void_p), n)
    return rc, list(out)


def test_layout_is_consistent():
    lib = L.load()
    sizes = (0, 1, 4095, 4096, 4097, 3 * 4096 + 17, 2 ** 20, 2 ** 20 + 1, 513 * 4096 + 5,
             2 ** 30, 2 ** 40 + 3)
    for n_rows in sizes:
        for k in sorted({0, 1, 5, 255, 5000, max(n_rows - 1, 0), n_rows, n_rows + 5, 2 ** 41}):
            rc, out = _layout(lib, n_rows, k)
            assert rc == 7 and out[7] == -7, (n_rows, k)
            ctl, bins, tile, ckey, crow, total, per_tile = out[:7]
            assert per_tile == TILE
            tiles, slots = (n_rows + per_tile - 1) // per_tile, min(k, n_rows)
            assert all(v % 8 == 0 for v in out[:6])
            # five 64-bit control words, 256 bins, two counts per tile, the slots
            assert ctl == 0 and bins - ctl >= 40 and tile - bins >= 8 * 256
            assert ckey - tile >= 16 * tiles and crow - ckey >= 8 * slots
            assert total - crow >= 8 * slots
            assert total == lib.tpe_pool_topk_scratch_bytes(n_rows, k)
    # fewer entries than seven: that many are written
    rc, out = _layout(lib, 5000, 9, 3)
    assert rc == 3 and out[3:] == [-7] * 5 and out[:3] == _layout(lib, 5000, 9)[1][:3]
    assert lib.tpe_pool_topk_layout(5000, 9, None, 0) == 0


def test_layout_argument_errors():
    """Host only: bad arguments are reported without a device."""
    lib = L.load()
    for n_rows, k, n in ((-1, 1, 7), (1, -1, 7), (1, 1, -1)):
        assert _layout(lib, n_rows, k, n)[0] == -1, (n_rows, k, n)
        assert b"tpe_pool_topk_layout" in lib.tpe_last_error()
    assert lib.tpe_pool_topk_layout(5000, 9, None, 7) == -1
    assert b"tpe_pool_topk_layout" in lib.tpe_last_error()
    assert lib.tpe_pool_topk_scratch_bytes(-1, 1) == -1
