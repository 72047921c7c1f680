"""Distinct configurations on the host (no GPU): the numpy reference of
tests/test_gpu_distinct.py against np.unique, and the argument checks and the
scratch query of tpe_pool_distinct."""
import ctypes

import numpy as np
import pytest

from hyperopt_amd import _lib as L
from hyperopt_amd import tpe
from tests.test_gpu_distinct import _canonical, config_first, reference_first


def _unique_first(vals, active):
    """first[r] by np.unique over the rows' canonical bytes (a void view)."""
    rows = np.where(active, _canonical(vals), 0.0)
    packed = np.ascontiguousarray(np.concatenate([rows.view(np.uint8).reshape(len(rows), -1),
                                                  active.astype(np.uint8)], axis=1))
    void = packed.view(np.dtype((np.void, packed.shape[1]))).reshape(-1)
    _, index, inverse = np.unique(void, return_index=True, return_inverse=True)
    return index[np.asarray(inverse).reshape(-1)]


@pytest.mark.parametrize("seed", range(6))
def test_reference_matches_np_unique(seed):
    rng = np.random.RandomState(seed)
    n, nl = rng.randint(1, 200), rng.randint(1, 6)
    vals = np.array([0.0, -0.0, 1.0, np.nan, -2.5])[rng.randint(0, 5, (n, nl))]
    active = rng.rand(n, nl) < 0.7
    noisy = np.where(active, vals, rng.normal(size=vals.shape))  # dead entries are ignored
    first = reference_first(noisy, active)
    np.testing.assert_array_equal(first, _unique_first(vals, active))
    # seen rows: rows [0, T) of the same set seen, the rest as a pool
    T = n // 3
    got = reference_first(noisy[T:], active[T:], noisy[:T], active[:T])
    for r, f in enumerate(got):
        whole = first[T + r]
        assert f == (-1 - whole if whole < T else whole - T)
    assert config_first([{"a": 1}, {"a": 1.0}, {"b": 1}], [{"b": 1}]).tolist() == [0, 0, -1]


def test_pool_distinct_checks_arguments():
    """tpe_pool_distinct reports argument errors before any launch and returns
    0 when there is nothing to do."""
    lib = L.load()
    one = ctypes.c_void_p(8)  # a non-null stand-in: validation fails before any launch

    def call(n_rows=10, n_labels=2, ld=10, n_seen=0, seen_ld=0, hash_bits=64, ptr=one, first=one,
             shift=None):
        return lib.tpe_pool_distinct(ptr, ptr, ld, n_rows, n_labels, ptr, ptr, seen_ld, None,
                                     n_seen, shift, hash_bits, None, first, None, one, None)
    assert call(n_rows=0, ptr=None, first=None) == 0  # nothing to do
    for kw in (dict(n_rows=-1), dict(n_seen=-1), dict(n_labels=-1), dict(hash_bits=-1),
               dict(hash_bits=65), dict(ld=-1)):
        assert call(**kw) == -1, kw
        assert b"tpe_pool_distinct" in lib.tpe_last_error()
    assert call(first=None) == -1 and b"null pointer" in lib.tpe_last_error()
    assert call(ptr=None) == -1 and b"null pointer" in lib.tpe_last_error()
    assert call(ld=9) == -1 and b"ld=9" in lib.tpe_last_error()
    assert call(n_seen=5, seen_ld=4) == -1 and b"seen_ld=4" in lib.tpe_last_error()
    far = np.zeros(5000)
    far[4999] = 1.0
    assert call(n_labels=5000, n_seen=5, seen_ld=5, shift=far.ctypes.data) == L.E_UNSUPPORTED
    assert b"shift" in lib.tpe_last_error()
    assert tpe.distinct_rows is not None


def test_pool_distinct_scratch_query():
    lib = L.load()
    q = lib.tpe_pool_distinct_scratch_bytes
    assert q(-1, 0) == -1 and q(0, -1) == -1 and q(1 << 60, 0) == -1
    assert q(0, 0) > 0
    sizes = [0, 1, 63, 64, 65, 1000, 4097, 1 << 20]
    for P in sizes:
        for T in sizes:
            assert q(P, T) >= 16 * 2 * (P + T) + 8 * P, (P, T)
    for P in sizes:
        got = [q(P, T) for T in sizes]
        assert got == sorted(got)
        got = [q(T, P) for T in sizes]
        assert got == sorted(got)
