"""Every draw of the library against the numpy replay of its Philox streams
(oracle/streams.py, itself pinned by tests/test_oracle_streams.py): candidate
g of a label IS the documented function of (key, g, attempt) -- generator,
counter layout, word use, component choice, Box-Muller pairing, retries and
the clamp -- for the fp64 and fp32 candidate streams, quantized slots,
categorical candidates, prior draws and the annealing pick and value.

The cases (tests/stream_cases.py) reach the paths the statistical tests never
do: mixtures on both sides of the staging limit, guide buckets with several
thresholds, a wave's retry list overflowing, many retry calls, the clamp,
threads starting inside a Philox quad, and indices at and above 2^32.
"""
import ctypes

import numpy as np
import pytest

from oracle import streams as S
from oracle import tpe_oracle as O
from tests import stream_cases as C

pytestmark = pytest.mark.gpu

_P = ctypes.c_void_p


# ---------------------------------------------------------------------------
# harness: explicit mixtures through hyperopt_amd.mixture._Mixture
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixtures():
    """name -> (_Mixture, cdf, mu, sigma): the arrays read back from the
    device, so the replay uses the device's own cumulative weights."""
    from hyperopt_amd import _lib as L
    from hyperopt_amd.mixture import _Mixture
    cache = {}

    def get(name):
        if name not in cache:
            c = C.case(name)
            m = _Mixture(L.LGMM1 if c.family == "LGMM1" else L.GMM1, c.w, c.mu, c.sigma, None,
                         None)
            cdf, mu, sig = (t.cpu().numpy() for t in (m.d_cdf, m.d_mu, m.d_sigma))
            h_cdf, h_mu, h_sig = C.host_cdf(c)
            assert np.array_equal(mu, h_mu) and np.array_equal(sig, h_sig)
            np.testing.assert_allclose(cdf, h_cdf, rtol=1e-14, atol=1e-15)
            cache[name] = (m, cdf, mu, sig)
        return cache[name]
    return get


def _sample(m, c, precision, base, q=None):
    """tpe_sample as _Mixture.sample issues it, with the job's cand_base set."""
    from hyperopt_amd import _lib as L
    flags = (L.F_LOW | L.F_HIGH) if c.low is not None else 0
    if q is not None:
        flags |= L.F_QUANT
    job = m.job(c.n, flags, c.low, c.high, q, c.key)
    job["cand_base"] = base
    d_job = m.upload(job)
    out = m.torch.empty(c.n, dtype=m.torch.float64, device=m.dev)
    _, mu, s, cdf, _, _ = m.ptrs()
    L.check(m.lib.tpe_sample(_P(d_job.data_ptr()), job.ctypes.data_as(_P), 1,
                             _P(m.d_seg.data_ptr()), mu, s, cdf, precision,
                             _P(out.data_ptr()), _P(m.stream.cuda_stream)), "tpe_sample")
    return out.cpu().numpy()


def _coordinate(c, x):
    return np.log(x) if c.family == "LGMM1" else x


# ---------------------------------------------------------------------------
# the fp64 stream
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CASES, ids=C.CASE_IDS)
def test_fp64_stream(c, mixtures):
    """|y_dev - y_ref| <= 1e-13 (|mu_k| + sigma_k max(1, |z|)) in the mixture
    coordinate; clamped draws are the bound itself.  Measured on MI355X: the
    largest error over all cases and bases is 0.008 of the bound (8e-16 of
    the scale; case loguniform-64)."""
    m, cdf, mu, sig = mixtures(c.name)
    worst = 0.0
    for base in C.BASES:
        y = _coordinate(c, _sample(m, c, 64, base))
        rep = S.gmm_draw64(cdf, mu, sig, c.key, C.indices(c, base), c.low, c.high)
        amb = C.ambiguous64(c, rep)
        assert amb.sum() <= C.CAP64, (base, int(amb.sum()))
        ok = ~amb
        err, tol = np.abs(y - rep["y"]), C.tol64(rep, mu, sig)
        ratio = float(np.max(err[ok] / tol[ok]))
        worst = max(worst, ratio)
        bad = ok & ~(err <= tol)
        assert not bad.any(), (base, int(bad.sum()), np.flatnonzero(bad)[:5], ratio)
        cl = ok & rep["clamped"]
        if c.family == "GMM1":
            assert np.array_equal(y[cl], rep["y"][cl]), base
        if c.low is not None:
            assert y.min() >= c.low and y.max() < c.high
    print("fp64 %s: max err / tol = %.3g" % (c.name, worst))


# ---------------------------------------------------------------------------
# the fp32 stream
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CASES, ids=C.CASE_IDS)
def test_fp32_stream(c, mixtures):
    """|y_dev - (mu32_k + sigma32_k z_ref)| <= 1e-4 sigma32_k max(1, |z_ref|)
    + 2 ulp32(y): the device's Box-Muller runs on v_log_f32 / v_sqrt_f32 /
    v_cos_f32 / v_sin_f32 and fp32 residuals, the replay in fp64.  A wrong
    word, component, pair member or attempt is off by O(sigma).  Measured on
    MI355X over all cases and bases: max |z_dev - z_ref| = 2.4e-5 (0.23 of
    the bound; case uniform-63, a candidate whose radius residual is
    1 - 2.3e-6: its fp32 rounding, 5e-8, over the radius 0.0022 is 2.4e-5),
    1.2e-5 in the next worst case and 1e-6 .. 9e-6 in the others."""
    m, cdf, mu, sig = mixtures(c.name)
    worst_z = worst = 0.0
    where = None
    for base in C.BASES:
        y = _coordinate(c, _sample(m, c, 32, base))
        rep = S.gmm_draw32(cdf, mu, sig, c.key, C.indices(c, base), c.low, c.high)
        amb = C.ambiguous32(c, rep)
        assert amb.sum() <= C.CAP32 * c.n, (base, int(amb.sum()))
        ok = ~amb
        err, tol = np.abs(y - rep["y"]), C.tol32(rep, y)
        free = ok & ~rep["clamped"]
        if free.any():
            dz = np.where(free, err / rep["sigma32"][rep["comp"]], 0.0)
            if dz.max() > worst_z:
                i = int(np.argmax(dz))
                worst_z, where = float(dz[i]), (base, i, float(rep["z"][i]))
        worst = max(worst, float(np.max(err[ok] / tol[ok])))
        bad = ok & ~(err <= tol)
        assert not bad.any(), (base, int(bad.sum()), np.flatnonzero(bad)[:5], worst)
        cl = ok & rep["clamped"]
        if c.family == "GMM1":
            assert np.array_equal(y[cl], rep["y"][cl]), base
        if c.low is not None:
            lo32, hi32 = float(np.float32(c.low)), float(np.float32(c.high))
            assert y.min() >= lo32 - 1e-6 * abs(lo32) and y.max() < hi32 + 1e-6 * abs(hi32)
        # the case reaches the path it is named for
        if c.tag == "half":
            assert C.max_wave_rejections(rep) > C.RETRY_LIST
        if c.tag == "r97":
            assert rep["calls"].max() >= 3
        if c.tag == "clamp":
            assert rep["clamped"].all()
    print("fp32 %s: max |z_dev - z_ref| = %.3g at (base, index, z_ref) = %s, max err / tol = %.3g"
          % (c.name, worst_z, where, worst))


# ---------------------------------------------------------------------------
# quantized slots
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name,q", C.QUANT)
def test_quantized_indices(name, q, precision, mixtures):
    """rint(v / q) of the fp64 stream and of the fp32 (TPE_F_DRAW32) stream
    -- LGMM1 through the fast fp32 exponential -- equals the replay's, except
    next to a half-integer."""
    c = C.case(name)
    m, cdf, mu, sig = mixtures(name)
    for base in C.BASES[:2]:
        x = _sample(m, c, precision, base, q=q)
        k_dev = np.rint(x / q)
        assert np.array_equal(k_dev * q, x)
        draw = S.gmm_draw64 if precision == 64 else S.gmm_draw32
        rep = draw(cdf, mu, sig, c.key, C.indices(c, base), c.low, c.high)
        if precision == 64:
            amb, tol = C.ambiguous64(c, rep), C.tol64(rep, mu, sig)
        else:
            amb, tol = C.ambiguous32(c, rep), C.tol32(rep, rep["y"])
        k_ref, half = C.quant_index(c, rep, q, tol, fast_exp=precision == 32)
        assert half.sum() <= C.CAP_Q * c.n
        ok = ~(amb | half)
        assert ok.sum() >= 0.98 * c.n
        assert np.array_equal(k_dev[ok].astype(np.int64), k_ref[ok]), \
            (base, np.flatnonzero(ok & (k_dev != k_ref))[:5])
        print("quantized %s q=%g fp%d base=%d: %d half-integer, %d bound-ambiguous of %d"
              % (name, q, precision, base, int(half.sum()), int(amb.sum()), c.n))


# ---------------------------------------------------------------------------
# the same fp32 stream from the scorers
# ---------------------------------------------------------------------------
def test_scorers_draw_the_sampler_stream_past_the_retry_list():
    """A label with about half of its below mass outside the bounds: the
    table scorer (draw32_pairs) and the fast table scorer (lean_draw, 32
    candidates per thread) return sample_only's candidates bit for bit, with
    waves whose rejections overflow the retry list; and those candidates are
    the replay's."""
    from hyperopt_amd.engine import Engine, LabelWork
    eng = Engine()
    rng = np.random.RandomState(50)
    below, above = rng.uniform(0.0, 0.02, 25), rng.uniform(0.0, 10.0, 200)
    key = 0x7E57_0000_0000_0032
    for base in (0, 2 ** 32 - 2050):
        w = LabelWork("x", "uniform", (0.0, 10.0), below, above, n_cand=C.N_CAND, key=key,
                      cand_base=base, n_total=1 << 16)  # a shard of a table-sized label
        s, = eng.run([w], precision=32, sample_only=True)
        tab, = eng.run([w], precision=32, outputs=True, scorer="table")
        fast, = eng.run([w], precision=32, table_scores=True)
        assert np.array_equal(tab.cand, s.cand)
        assert np.array_equal(fast.cand, s.cand)
        post, = eng.run([w], posteriors=True)
        wb, mu, sig = post.extra["below"]
        rep = S.gmm_draw32(np.cumsum(wb) / np.sum(wb), mu, sig, key,
                           base + np.arange(C.N_CAND, dtype=np.int64), 0.0, 10.0)
        assert C.max_wave_rejections(rep, 1024) > C.RETRY_LIST   # 16 candidates per thread
        assert C.max_wave_rejections(rep, 2048) > C.RETRY_LIST   # 32 candidates per thread
        c = C.Case("label", "GMM1", wb, mu, sig, 0.0, 10.0, key, C.N_CAND, "half")
        amb = C.ambiguous32(c, rep)
        assert amb.sum() <= C.CAP32 * C.N_CAND
        err, tol = np.abs(s.cand - rep["y"]), C.tol32(rep, s.cand)
        assert np.all(err[~amb] <= tol[~amb]), int(np.sum(err[~amb] > tol[~amb]))


# ---------------------------------------------------------------------------
# categorical candidates
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 8, 40, 256, 257, 300])
def test_categorical_stream(K):
    """Every drawn category is word g & 3 of call g >> 2 against the
    thresholds of the device's own cumulative p -- registers, binary search
    and the plain path (K around 4 / 8 / 16 and 256), aligned and unaligned
    bases, indices across 2^32."""
    from hyperopt_amd.engine import Engine, LabelWork
    eng = Engine()
    rng = np.random.RandomState(K)
    obs_b, obs_a = rng.randint(0, K, 25), rng.randint(0, K, 400)
    p_ref = O.randint_posterior(obs_b, 1.0, K)
    key = 0xCA7_0000_0000 + K
    for n_cand in (1001, 4096 * 16 + 3):
        for base in (0, 3, 2 ** 32 - 2):
            w = LabelWork("c", "randint", (K,), obs_b, obs_a, n_cand=n_cand, key=key,
                          cand_base=base, n_total=n_cand)
            r, = eng.run([w], outputs=True)
            cdf = eng._bufs["cat_cdf"][:8 * K].cpu().numpy().view(np.float64).copy()
            np.testing.assert_allclose(np.diff(np.concatenate([[0.0], cdf])), p_ref, rtol=0,
                                       atol=1e-14)  # the below segment's cumulative p
            want = S.categorical_draw(cdf, key, base + np.arange(n_cand, dtype=np.int64))
            assert np.array_equal(r.cand.astype(np.int64), want), (n_cand, base)
            s = r.below_llik - r.above_llik
            best = int(np.argmax(s))
            assert (r.index, int(r.value)) == (base + best, int(want[best]))


# ---------------------------------------------------------------------------
# prior draws
# ---------------------------------------------------------------------------
def test_prior_stream():
    """tpe_prior_sample at base 0 and across 2^32: uniform, quniform, randint
    and pchoice exactly (the same IEEE operations; uniform(0, 1) returns
    u01_f64 itself, all 53 bits), the log / exp / Box-Muller kinds within
    1e-13 of their terms' magnitude, their quantized forms exactly except next
    to a half-integer."""
    import torch
    from hyperopt_amd import _lib as L
    labels, rec, pool = C.prior_records()
    assert len(set(rec["key"].tolist())) == len(labels)
    n = C.PRIOR_N
    dev = torch.device("cuda", torch.cuda.current_device())
    d_rec = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    d_p = torch.from_numpy(pool).to(dev)
    stream = torch.cuda.current_stream(dev)
    seen = set()
    for base in C.PRIOR_BASES:
        out = torch.empty(len(labels) * n, dtype=torch.float64, device=dev)
        L.check(L.load().tpe_prior_sample(d_rec.data_ptr(), rec.ctypes.data_as(_P), len(labels),
                                          d_p.data_ptr(), n, base, out.data_ptr(),
                                          _P(stream.cuda_stream)), "tpe_prior_sample")
        got = out.cpu().numpy().reshape(len(labels), n)
        idx = base + np.arange(n, dtype=np.int64)
        for j, lab in enumerate(labels):
            R = rec[j]
            d = S.prior_draw(R, pool, int(R["key"]), idx)
            kind, q = int(R["kind"]), float(R["q"])
            seen.add((kind, q > 0))
            x = got[j]
            if not C.prior_is_smooth(R):
                assert np.array_equal(x, d["v"]), (lab, base)
                continue
            tol = C.prior_tol(R, d)
            if q == 0.0:
                err = np.abs(x - d["raw"])
                assert np.all(err <= tol), (lab, base, np.max(err / tol))
                continue
            half = C.prior_half(R, d)
            assert half.sum() <= C.CAP_PRIOR, (lab, base)
            assert np.array_equal(x[~half], d["v"][~half]), (lab, base)
    assert len(seen) == 10  # every kind, quantized and not


# ---------------------------------------------------------------------------
# annealing: the pick and the value
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("avg_best_idx", C.ANNEAL_AVG)
def test_anneal_stream(avg_best_idx):
    """The rank g is anneal_pick(key, new_id) (counter word 0) and the value's
    variate anneal_variate (counter word 1) for trial ids across 2^32; the
    chosen row is then rows[argsort(loss)[g]] with the REPLAYED g."""
    from hyperopt_amd import _lib as L
    from hyperopt_amd import anneal, tpe
    from hyperopt_amd.engine import DeviceHistory
    n_trials, ids = C.ANNEAL_TRIALS, C.ANNEAL_IDS
    eng = tpe.engine()
    losses, active, vals, keys = C.anneal_history()
    dh = DeviceHistory(eng, 3, cap=16)
    dh.append(vals, active)
    loss = eng.torch.from_numpy(losses).to(dh.device)
    rec = np.zeros(3, L.ANNEAL_DTYPE)
    rec["kind"] = C.ANNEAL_KINDS
    rec["a"], rec["b"] = 0.0, 1.0
    rec["col"] = np.arange(3)
    rec["n_active"] = active.sum(0)
    rec["shrink"] = 1.0 / (1.0 + 0.1 * rec["n_active"])
    rec["key"] = keys
    items = [[t % 3] for t in range(n_trials)]  # one label per trial: every item is a new pick
    state = anneal.chain_state(eng, dh, rec, np.zeros(1), ids)
    out, dbg = anneal.sample_level(eng, dh, loss, rec, None, items, ids, avg_best_idx, state,
                                   debug=True)
    assert state["err"] == 0
    for j in range(3):
        t = np.arange(j, n_trials, 3)
        key, kind = int(rec["key"][j]), int(rec["kind"][j])
        g, quo = S.anneal_pick(key, ids[t], avg_best_idx, int(rec["n_active"][j]))
        # cap 0: no id's quotient sits on an integer
        assert not np.any(np.abs(quo - np.rint(quo)) <= C.ANNEAL_QUOTIENT_TOL)
        assert np.array_equal(dbg["g"][t], g), j
        rows = np.flatnonzero(active[:, j])
        order = np.argsort(losses[rows], kind="stable")
        assert np.array_equal(dbg["row"][t], rows[order[g]]), j
        assert np.all(dbg["reused"][t] == 0)
        v = S.anneal_variate(key, ids[t], kind)
        if kind == L.PRIOR_UNIFORM:
            assert np.array_equal(dbg["variate"][t], v), j
        else:
            assert np.all(np.abs(dbg["variate"][t] - v) <= 1e-13 * np.maximum(1.0, np.abs(v)))
    if avg_best_idx > 2:
        assert np.mean(dbg["g"][2::3] == 2) > 0.9  # the three-row column clips at its last row
