"""What the band tests share (test_gpu_band_tiles.py, test_gpu_band_paths.py):
the band work's layout and the two stages' constants from tpe_band_layout,
the band buffers of an engine read back, histories, and the exact references.
"""
import ctypes

import numpy as np

from hyperopt_amd import _lib as L
from oracle import tpe_oracle as O

CONT = [("uniform", (-5.0, 5.0)), ("loguniform", (-5.0, 0.0)), ("normal", (0.0, 2.0)),
        ("lognormal", (0.0, 1.0))]
LGMM = ("loguniform", "lognormal")

_NAMES = ("work_bytes", "o_ns", "o_ncell", "o_over", "o_direct", "o_sy", "o_sidx", "o_cells",
          "kBandBlocks", "kBandDirect", "kBandSurv", "kBandCells", "kBandSurvMax", "kBandTiles",
          "kChunkDir", "kTileSlots", "kTileF", "kHdrWords", "kTileFull")


class Layout(object):
    """tpe_band_layout's words by name."""

    def __init__(self):
        lib = L.load()
        n = lib.tpe_band_layout(None, 0)
        assert n == len(_NAMES), n
        out = (ctypes.c_int64 * n)()
        assert lib.tpe_band_layout(ctypes.cast(out, ctypes.c_void_p), n) == n
        for k, v in zip(_NAMES, out):
            setattr(self, k, int(v))


_layout = None


def layout():
    global _layout
    if _layout is None:
        _layout = Layout()
    return _layout


def n_tiles_of(n_cands):
    K = layout()
    return max(1, max((int(n) + K.kTileF - 1) // K.kTileF for n in n_cands))


def read_work(eng, n_jobs=1):
    """Each job's route, {ns, ncell, over, direct, cells}, from the engine's band work."""
    K = layout()
    small = (("ns", K.o_ns), ("ncell", K.o_ncell), ("over", K.o_over), ("direct", K.o_direct))
    a = min([K.o_cells] + [o for _, o in small])
    b = max([K.o_cells + 4 * K.kBandCells] + [o + 4 for _, o in small])
    out = []
    for j in range(n_jobs):
        w = eng._bufs["band_work"][j * K.work_bytes + a:j * K.work_bytes + b].cpu().numpy()
        f = {k: int(w[o - a:o - a + 4].view(np.int32)[0]) for k, o in small}
        f["cells"] = w[K.o_cells - a:K.o_cells - a + 4 * K.kBandCells].view(np.int32).copy()
        out.append(f)
    return out


def read_tiles(eng, n_jobs, n_tiles):
    """(headers [job, tile] as {lo, hi_max: float32, n: uint32}, entries [job, tile, slot])
    of the engine's band buffers."""
    K = layout()
    ctl = eng._bufs["band_ctl"][:4 * K.kHdrWords * n_jobs * n_tiles].cpu().numpy() \
        .view(np.uint32).reshape(n_jobs, n_tiles, K.kHdrWords).copy()
    band = eng._bufs["band"][:L.BAND_DTYPE.itemsize * K.kTileSlots * n_jobs * n_tiles].cpu() \
        .numpy().view(L.BAND_DTYPE).reshape(n_jobs, n_tiles, K.kTileSlots).copy()
    hdr = {"lo": ctl[:, :, 0].copy().view(np.float32), "hi_max": ctl[:, :, 1].copy().view(np.float32),
           "n": ctl[:, :, 2].copy()}
    return hdr, band


def history(kind, args, n_hist, seed):
    """A natural history's below / above lists: n_hist draws from the prior,
    split by random losses (gamma = 0.25)."""
    from tests.test_gpu_parity import _mixture_case
    rng = np.random.RandomState(seed)
    obs = _mixture_case(rng, kind, args, 1, n_hist, 1).obs_above
    losses = rng.normal(size=n_hist)
    return O.ap_split_trials(np.arange(n_hist), obs, np.arange(n_hist), losses, 0.25)


def cand_value(y, kind):
    """The value of a candidate drawn as y (fp32): y, or exp(y) in fp64."""
    y = np.asarray(y, np.float32).astype(np.float64)
    return np.exp(y) if kind in LGMM else y


def assert_value_is(value, y, kind):
    """``value`` is the device's cand_value(y).  GMM1: the same number.  LGMM1:
    exp in fp64, whose last bit may differ between the device's exp and
    numpy's, so: within 2 ulp of numpy's, and the fp32 nearest to its log is
    y -- which no other fp32 draw satisfies (|log(exp(y)) - y| <= 2^-51 (1 +
    |y|), far below half an fp32 ulp)."""
    value, y = np.asarray(value, np.float64), np.asarray(y, np.float32)
    if kind not in LGMM:
        np.testing.assert_array_equal(value, y.astype(np.float64))
        return
    np.testing.assert_allclose(value, np.exp(y.astype(np.float64)), rtol=4.5e-16, atol=0)
    with np.errstate(all="ignore"):
        np.testing.assert_array_equal(np.log(value).astype(np.float32), y)


def dense64(eng64, kind, args, below, above, cand):
    """The dense fp64 kernel's scores of ``cand`` (test_gpu_parity pins its
    log-densities to the oracle at rtol 1e-6) and their np.argmax."""
    from hyperopt_amd.engine import LabelWork
    assert eng64.exact64 == "dense"
    x, = eng64.run([LabelWork(kind, kind, args, below, above, cand=np.asarray(cand, np.float64))],
                   precision=64, outputs=True)
    s64 = x.below_llik - x.above_llik
    best = int(np.argmax(s64))
    assert x.index == best
    return s64, best


def oracle_scores(kind, args, below, above, cand):
    with np.errstate(all="ignore"):
        r = O.continuous_label_scores(kind, args, below, above, np.asarray(cand, np.float64))
    return r["below_llik"] - r["above_llik"]
