"""The device code of the categorical counts' exact fold
(hyperopt_amd/csrc/tpe_fold.hpp) on lists the LF ramp never produces, through
tpe_fold_check: one wave (scope 0: the driver of k_cat_counts and
k_cat_counts_hist) and one block (scope 1: k_cath_fold's) fold each list of
tests/fold_cases.py -- LF ramps, tie-heavy dyadic weights, 24-decade ranges,
sums started at 2^53 / 2^52+1 / 1e16 / 1e-300 / 5e-324 -- and lists on the
pass and staging edges, with the serial prefix taken whole (done = 0), ended
inside the list (4000) and skipped (4096).  Every sum must be the bits of the
serial chain s = s + w in numpy float64, computed on the host."""
import ctypes

import numpy as np
import pytest

from tests import fold_cases

pytestmark = pytest.mark.gpu

EDGES = {0: (1, 511, 512, 513, 1025), 1: (1, 4095, 4096, 4097, 8193)}
_REF = {}


def _cases(scope):
    return (fold_cases.lf_ramp_cases() + fold_cases.adversarial_cases()
            + fold_cases.edge_cases(EDGES[scope]))


def _reference(scope):
    """The serial chains, once per scope's case list (they do not depend on
    `done`: it only moves the hand-over from the serial prefix to the passes)."""
    if scope not in _REF:
        _REF[scope] = [fold_cases.serial(S0, w) for _, S0, w in _cases(scope)]
    return _REF[scope]


@pytest.mark.parametrize("done", [0, 4000, 4096])
@pytest.mark.parametrize("scope", [0, 1])
def test_fold_matches_the_serial_chain(scope, done):
    import torch
    from hyperopt_amd import _lib as L
    lib = L.load()
    cases = _cases(scope)
    offs = np.concatenate([[0], np.cumsum([len(w) for _, _, w in cases])])
    flat = torch.from_numpy(np.concatenate([np.asarray(w, np.float64) for _, _, w in cases]))
    dev = flat.cuda()
    out = torch.full((len(cases),), -1.0, dtype=torch.float64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for i, (_, S0, w) in enumerate(cases):  # one launch per case
        L.check(lib.tpe_fold_check(dev.data_ptr() + 8 * int(offs[i]), len(w), S0, done, scope,
                                   out.data_ptr() + 8 * i, st), "tpe_fold_check")
    got = out.cpu().numpy()
    want = np.array(_reference(scope))
    bad = [(cases[i][0], float(got[i]).hex(), float(want[i]).hex())
           for i in np.flatnonzero(got != want)]
    assert not bad, (scope, done, len(bad), bad[:5])
