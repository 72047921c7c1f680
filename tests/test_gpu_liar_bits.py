"""The three liar batches against the bits recorded before they shared one
engine (tests/golden/liar_bits.npz, written by tools/record_liar_bits.py): the
rows, ``S_at_pick`` and ``S_k`` of ``liar_device``, ``liar_tree_device`` and
``liar_chain_device`` on the seeded cases of test_gpu_liar_tree.py and
test_gpu_liar_chain.py (a NaN score, -inf in A / B, both masks).

The cross-mode tests there compare one call with another; since the three are
one kernel they would pass if all three moved together.  This file would not.
"""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "liar_bits.npz")
SIZES = [(1, 1), (257, 3), (600, 602)]
# (entry, shape): the shapes are those of the entry's own GPU test file
ENTRIES = [("flat", "flat"), ("tree", "flat"), ("tree", "tree"), ("chain", "chain"),
           ("chain", "branch")]
CASES = [(entry, shape, P, k) for entry, shape in ENTRIES for P, k in SIZES]


def case_id(entry, shape, P, k):
    return "%s-%s-%d-%d" % (entry, shape, P, k)


def run(entry, shape, P, k):
    """(rows, S_at_pick, S_k) of one device entry with ``trace=True``."""
    if entry == "chain":
        from tests.test_gpu_liar_chain import _device
        return _device(shape, P, k)
    from tests.test_gpu_liar_tree import _device
    return _device(shape, P, k, flat=entry == "flat")


def parts(entry, shape, P, k):
    """What is recorded of a case: name -> array, the doubles as uint64."""
    rows, at, S_k = run(entry, shape, P, k)
    name = case_id(entry, shape, P, k)
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)  # noqa: E731
    return {name + "/rows": np.asarray(rows, np.int64), name + "/S_at_pick": bits(at),
            name + "/S_k": bits(S_k)}


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {name: z[name] for name in z.files}


@pytest.mark.parametrize("entry,shape,P,k", CASES, ids=[case_id(*c) for c in CASES])
def test_recorded_bits(golden, entry, shape, P, k):
    got = parts(entry, shape, P, k)
    assert len(got[case_id(entry, shape, P, k) + "/rows"]) in (k, 23, 24)
    for name, a in got.items():
        want = golden[name]
        assert a.dtype == want.dtype and a.shape == want.shape, name
        assert (a == want).all(), (name, int((a != want).sum()))


@pytest.mark.parametrize("P,k", SIZES)
def test_the_tree_entry_has_the_recorded_bits(golden, P, k):
    """``liar_tree_device`` goes through tpe_joint_lie_chain_picks; the C ABI's
    tpe_joint_lie_tree_picks itself, on the "tree" shape."""
    import torch as t
    from hyperopt_amd import _lib as L
    from hyperopt_amd import joint as J
    from hyperopt_amd import pool as pool_mod
    from hyperopt_amd import tpe
    from tests import test_gpu_liar_tree as T
    domain, trials, pool, _sets, _live, S0, A, gone = T._case("tree", P)
    eng, lib = tpe.engine(), L.load()
    d = pool.device(eng)
    fits = pool_mod._fit(eng, domain, tpe.collect_history(trials, pool.labels), len(pool.labels),
                         pool_mod._settings(1.0, 0.25, 25, "tree", T.BW, T.SMOOTHING))
    pk, G = J._lie_pack(fits), len(fits)
    up = lambda a: t.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    odd = (np.arange(P) % 2).astype(np.uint8)
    S0_d, A_d, taken, distinct = up(S0), up(A.T), up(gone * odd), up(gone * (1 - odd))
    name, k = case_id("tree", "tree", P, k), min(k, P)
    out = t.empty(k + 1, dtype=t.int64, device=eng.device)
    at, S_k = (t.empty(n, dtype=t.float64, device=eng.device) for n in (k, P))
    scratch = t.empty(lib.tpe_joint_lie_tree_scratch_bytes(P, G), dtype=t.uint8, device=eng.device)
    assert scratch.numel() == lib.tpe_joint_lie_chain_scratch_bytes(P, G, 0)
    L.check(lib.tpe_joint_lie_tree_picks(
        pk.host.ctypes.data, pk.dev.data_ptr(), len(pk.host), pk.tables.data_ptr(), pk.n_tables,
        pk.off.ctypes.data, pk.log_w.ctypes.data, pk.col.ctypes.data, G, pk.sigma.data_ptr(),
        d.vals.data_ptr(), d.active.data_ptr(), d.vals.shape[1], d.vals.shape[0], P,
        S0_d.data_ptr(), A_d.data_ptr(), A_d.shape[1], math.log(T.LIE), taken.data_ptr(),
        distinct.data_ptr(), k, out.data_ptr(), out.data_ptr() + 8 * k, at.data_ptr(),
        S_k.data_ptr(), scratch.data_ptr(), J.stream_ptr(eng)), "tpe_joint_lie_tree_picks")
    got = out.cpu().numpy()
    rows = got[:int(got[k])]
    bits = lambda a: a.cpu().numpy().view(np.uint64)  # noqa: E731
    assert rows.tolist() == golden[name + "/rows"].tolist()
    assert (bits(at)[:rows.size] == golden[name + "/S_at_pick"]).all()
    assert (bits(S_k) == golden[name + "/S_k"]).all()
