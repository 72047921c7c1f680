"""Rows drawn from the joint below mixture on the GPU (csrc/tpe_joint_sample.hip
through its C entry point, tpe.Pool.sample(joint=True) and
tpe.suggest_sampled(joint=True, draw="joint")).

Reference: the numpy replay of the draw rule in tests/joint_sample_util.py,
under the comparison rules of tests/stream_cases.py for fp64 draws --
components, discrete values, clamped and quantized draws exactly; continuous
values within RTOL64 of |mu| + sigma max(1, |z|) in the fit coordinate; rows
whose replayed draw lies that close to a bound or to a half-integer of the
lattice left out, at most CAP64 per label and case (counted from the replay
alone in tests/test_joint_sample_host.py).  The distribution checks are that
file's, on the device's draws of the same rows, at p > 1e-4.
"""
import ctypes
from functools import partial

import numpy as np
import pytest

from hyperopt_amd import Domain, Trials, fmin, hp, rand, tpe
from hyperopt_amd import _lib as L
from hyperopt_amd import joint as J
from hyperopt_amd import pool as pool_mod
from tests import cond_util as C
from tests import joint_sample_util as R
from tests import joint_util as U
from tests import test_joint_sample_host as H
from tests.test_gpu_joint import KW, N_TRIALS
from tests.test_gpu_pool import _expected_order, _same_bits

pytestmark = pytest.mark.gpu

SEED = R.DIST_SEED


def _stream(eng):
    return ctypes.c_void_p(eng.torch.cuda.current_stream(eng.device).cuda_stream)


def _set_buffer(lib, models, mu, sig, cdf):
    """A prepared set written by hand in the header's layout: log w (C) | sigma
    (D) | 1 / (sqrt(2) sigma) (D) | pad to an even count | {mu, constant} (D x
    C, label-major; the sampler reads mu and sigma only)."""
    D, C = len(models), cdf.size
    n = C - 1
    buf = np.zeros(lib.tpe_joint_set_doubles(D, n))
    w = np.diff(np.concatenate([[0.0], cdf]))
    buf[:C] = np.log(w / cdf[-1])
    buf[C:C + D] = sig
    buf[C + D:C + 2 * D] = [1.0 / (np.sqrt(2.0) * s) if s > 0 else 0.0 for s in sig]
    off = (C + 2 * D + 1) & ~1
    comp = buf[off:].reshape(D, C, 2)
    comp[:, :n, 0] = np.asarray(mu, np.float64).reshape(D, n)
    comp[:, n, 0] = [-1.0 if m.kind == L.JOINT_CAT else m.mu for m in models]
    return buf


def _sample_abi(models, mu, sig, cdf, keys, comp_key, one_plus_a, row_base, n_rows, pad=3):
    """(vals (n_cols, ld), comp) of one tpe_joint_sample call on a hand-written
    set; ld = n_rows + pad, NaN where the kernel must not write."""
    eng = tpe.engine()
    t, lib = eng.torch, eng.lib
    dj = J._device_labels(eng, models, 1.0)
    n_cols = max(m.col for m in models) + 1
    ld = n_rows + pad
    up = lambda a: t.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    dset = up(_set_buffer(lib, models, mu, sig, cdf))
    dcdf = up(np.asarray(cdf, np.float64))
    cats = [np.cumsum(m.p) for m in models if m.kind == L.JOINT_CAT]
    dcat = up(np.concatenate(cats)) if cats else None
    dkeys = up(np.asarray(list(keys) + [comp_key], np.uint64).view(np.int64))
    vals = t.full((n_cols, ld), float("nan"), dtype=t.float64, device=eng.device)
    comp = t.full((max(n_rows, 1),), -7, dtype=t.int32, device=eng.device)
    L.check(lib.tpe_joint_sample(dj.host.ctypes.data, dj.dev.data_ptr(), len(models),
                                 dset.data_ptr(), cdf.size - 1, dcdf.data_ptr(),
                                 None if dcat is None else dcat.data_ptr(),
                                 0 if dcat is None else dcat.numel(), dkeys.data_ptr(),
                                 one_plus_a, row_base, n_rows, vals.data_ptr(), ld, n_cols,
                                 comp.data_ptr(), _stream(eng)), "tpe_joint_sample")
    return vals.cpu().numpy(), comp.cpu().numpy()[:n_rows]


def _run_case(c, row_base=None, n_rows=None):
    row_base = c["row_base"] if row_base is None else row_base
    n_rows = c["n_rows"] if n_rows is None else n_rows
    return _sample_abi(c["models"], c["mu"], c["sig"], c["cdf"], c["keys"], c["comp_key"],
                       c["one_plus_a"], row_base, n_rows)


# -- 1. the kernel against the replay, stage by stage -------------------------------
_CASES = R.stage_cases()


@pytest.mark.parametrize("c", _CASES, ids=[c["name"] for c in _CASES])
def test_stage_matches_replay(c):
    assert tpe.engine().lib.tpe_joint_sample_stage() == R.STAGE
    comp, out = R.replay_case(c)
    vals, dcomp = _run_case(c)
    n = c["n_rows"]
    np.testing.assert_array_equal(dcomp, comp)
    assert np.isnan(vals[:, n:]).all()  # nothing past the window
    worst = 0.0
    for m, rep in zip(c["models"], out):
        w, _ = R.compare(m, rep, vals[m.col, :n])
        worst = max(worst, w)
    print("%s: worst err / tol = %.3g" % (c["name"], worst))


def _all_kinds():
    domain, trials = H.all_kinds_case(N_TRIALS)
    return domain, trials, tpe.collect_history(trials, list(domain.params))


def test_all_kinds_through_the_prepared_set():
    """D = 12, every kind, the set built by tpe_joint_prep from the history."""
    domain, trials, hist = _all_kinds()
    eng = tpe.engine()
    t = eng.torch
    nl = len(domain.params)
    fit, = J.fit(eng, domain, hist, pool_mod._seen_rows(eng, hist), KW["gamma"], nl,
                 KW["prior_weight"], KW["linear_forgetting"], KW["bandwidth"],
                 KW["cat_smoothing"])
    n_rows, base = 300, 2 ** 32 - 3
    vals = t.full((nl, n_rows), float("nan"), dtype=t.float64, device=eng.device)
    comp = t.full((n_rows,), -7, dtype=t.int32, device=eng.device)
    J.sample_device(fit, SEED, vals, n_rows, nl, base, n_rows, comp_out=comp)
    models, rcomp, out = R.replay(domain, hist, SEED, base + np.arange(n_rows), **KW)
    np.testing.assert_array_equal(comp.cpu().numpy(), rcomp)
    got = vals.cpu().numpy()
    worst = max(R.compare(m, rep, got[m.col])[0] for m, rep in zip(models, out))
    print("all kinds: worst err / tol = %.3g" % worst)


# -- 2. bits do not depend on the launch ----------------------------------------------
def test_bits_do_not_depend_on_the_row_window():
    c = next(c for c in _CASES if c["name"] == "C26")
    base = c["row_base"]
    whole, comp = _run_case(c, base, 4096)
    lo, clo = _run_case(c, base, 2048)
    hi, chi = _run_case(c, base + 2048, 2048)
    win, cwin = _run_case(c, base + 1000, 300)
    for m in c["models"]:
        j = m.col
        assert _same_bits(np.concatenate([lo[j, :2048], hi[j, :2048]]), whole[j, :4096])
        assert _same_bits(win[j, :300], whole[j, 1000:1300])
    np.testing.assert_array_equal(np.concatenate([clo, chi]), comp)
    np.testing.assert_array_equal(cwin, comp[1000:1300])


# -- 3. distributions of the device's draws -------------------------------------------
def _born_columns(domain, trials, n, **kw):
    pool = tpe.Pool.sample(domain, trials, SEED, n, joint=True, **kw)
    return pool, pool._born().vals[:, :n].cpu().numpy()


def test_component_frequencies_follow_the_weights():
    models, mu, sig, cdf = H.component_case()
    _, comp = _sample_abi(models, mu, sig, cdf, [R._key(1)], J.component_key(SEED), 2.0, 0,
                          1 << 16)
    H.check_components(comp, cdf, 1e-4)


def test_diagonal_cells_and_the_share_of_the_diagonal():
    """The point of the feature.  The below set is the 16 diagonal trials: a
    trial component puts 0.625^2 + 3 x 0.125^2 = 0.4375 on a == b, the prior
    0.25, so (16 x 0.4375 + 0.25) / 17 = 0.4265 of the joint-drawn rows lie on
    the diagonal (binomial sd at 4096 rows: 0.0077); the factorised posteriors
    are flat there and give 0.25."""
    domain, trials = H.diagonal()
    pool, dv = _born_columns(domain, trials, R.DIST_ROWS, gamma=2.0)
    H.check_diagonal(dv[0], dv[1], 1e-4)
    share = float((dv[0, :4096] == dv[1, :4096]).mean())
    flat = tpe.Pool.sample(domain, trials, SEED, 4096, gamma=2.0)._born().vals.cpu().numpy()
    share_flat = float((flat[0] == flat[1]).mean())
    print("on the diagonal: joint %.4f, factorised %.4f" % (share, share_flat))
    assert 0.39 <= share <= 0.46
    assert share_flat <= 0.30


def test_quantized_lattice_follows_the_joint_below_mixture():
    domain, trials = H.one_label("quant")
    _, dv = _born_columns(domain, trials, R.DIST_ROWS)
    H.check_lattice(dv[0], 1e-4)


def test_bounded_label_follows_the_truncated_mixture():
    domain, trials = H.one_label("cont")
    _, dv = _born_columns(domain, trials, R.DIST_ROWS)
    H.check_ks(dv[0], 1e-4)


# -- 4. the public path ------------------------------------------------------------------
def test_pool_sample_joint_on_a_flat_space():
    domain, trials, hist = _all_kinds()
    n = 300
    kw = {k: KW[k] for k in ("prior_weight", "gamma", "linear_forgetting")}
    pool = tpe.Pool.sample(domain, trials, SEED, n, joint=True, keep_terms=True,
                           bandwidth=KW["bandwidth"], cat_smoothing=KW["cat_smoothing"], **kw)
    assert isinstance(pool, tpe.SampledPool) and len(pool) == n
    dv = pool._born().vals[:, :n].cpu().numpy()
    models, _, out = R.replay(domain, hist, SEED, np.arange(n), **KW)
    for m, rep in zip(models, out):
        R.compare(m, rep, dv[m.col])
    assert pool.active.all() and (pool.n_active == n).all()
    assert np.isnan(pool.terms()).all()  # every label is joint
    tpe.Pool.from_arrays(domain, pool.vals, pool.active)  # validates
    born = pool.scores().copy()
    assert not np.isnan(born).all()
    again = tpe.score_configs(domain, trials, pool, joint=True, **KW)
    assert _same_bits(born, again)
    # the same call gives the same pool; without joint= it gives today's
    twin = tpe.Pool.sample(domain, trials, SEED, n, joint=True, bandwidth=KW["bandwidth"],
                           cat_smoothing=KW["cat_smoothing"], **kw)
    assert _same_bits(twin._born().vals[:, :n].cpu().numpy(), dv)
    assert _same_bits(twin.scores(), born)
    plain = tpe.Pool.sample(domain, trials, SEED, n, **kw)
    assert not _same_bits(plain._born().vals[:, :n].cpu().numpy(), dv)


def _conditional():
    domain = Domain(lambda x: 0, C.shared_node(hp))
    trials = Trials()
    fmin(lambda cfg: float(cfg["k"]) + 0.1 * len(str(cfg)), C.shared_node(hp), algo=rand.suggest,
         max_evals=60, trials=trials, rstate=np.random.RandomState(3), show_progressbar=False)
    return domain, trials


def test_pool_sample_joint_on_a_conditional_space(monkeypatch):
    domain, trials = _conditional()
    labels = list(domain.params)
    n = 300
    jcols = [labels.index(lab) for lab in J.joint_labels(domain)]
    assert jcols == [labels.index("a")]
    rest = np.ones(len(labels), bool)
    rest[jcols] = False
    pool = tpe.Pool.sample(domain, trials, SEED, n, joint=True, keep_terms=True)
    plain = tpe.Pool.sample(domain, trials, SEED, n)
    dv = pool._born().vals[:, :n].cpu().numpy()
    # the labels under the switch: today's draws, bit for bit
    assert _same_bits(dv[rest], plain._born().vals[:, :n].cpu().numpy()[rest])
    hist = tpe.collect_history(trials, labels)
    models, _, out = R.replay(domain, hist, SEED, np.arange(n))
    R.compare(models[0], out[0], dv[jcols[0]])
    # activity: the program on the pool's own selector columns
    lo, co, tm = pool_mod.program_csr(domain)
    active = pool.active
    np.testing.assert_array_equal(active.T, C.interpret(lo, co, tm, dv, n))
    # keep_terms: NaN in the joint column, elsewhere where the label is not live
    terms = pool.terms()
    assert np.isnan(terms[:, jcols]).all()
    np.testing.assert_array_equal(np.isnan(terms[:, rest]), ~active[:, rest])
    born = pool.scores().copy()
    S, terms2, Jd = tpe.score_configs(domain, trials, pool, joint=True, return_terms=True)
    live = active & rest[None, :]
    scale = np.abs(Jd) + np.where(live, np.abs(terms2), 0.0).sum(1)
    err = np.abs(S - born)
    print("max |S_rescored - S_born| = %.3g" % err.max())
    assert (err <= 1e-6 * scale).all() and not _same_bits(born, Jd)
    # label chunks change nothing
    monkeypatch.setattr(pool_mod, "CHUNK_ELEMS", 2 * n)
    pool2 = tpe.Pool.sample(domain, trials, SEED, n, joint=True, keep_terms=True)
    assert _same_bits(pool2._born().vals[:, :n].cpu().numpy(), dv)
    assert _same_bits(pool2.scores(), born)
    np.testing.assert_array_equal(pool2.active, active)


def _doc_config(doc):
    return {k: v[0] for k, v in doc["misc"]["vals"].items() if v}


def _diagonal(drop=None):
    space, configs, losses = U.diagonal_case(hp)
    domain = Domain(lambda x: 0, space)
    if drop is not None:
        keep = [i for i, c in enumerate(configs) if 4 * c["a"] + c["b"] not in drop]
        configs, losses = [configs[i] for i in keep], [losses[i] for i in keep]
    return domain, U.make_trials(domain, configs, losses)


def test_suggest_sampled_draws_from_the_joint_mixture():
    domain, trials = _diagonal()
    ids = [100, 101, 102, 103, 104]
    kw = dict(n_EI_candidates=256, gamma=2.0, joint=True, verbose=False)
    docs = tpe.suggest_sampled(ids, domain, trials, SEED, draw="joint", **kw)
    pool = tpe.Pool.sample(domain, trials, SEED, 256, gamma=2.0, joint=True)
    S = pool.scores()
    rows = _expected_order(S, np.zeros(256), len(ids))
    assert [d["tid"] for d in docs] == ids  # k documents, the k best rows by the born S
    assert [_doc_config(d) for d in docs] == [pool.config(int(r)) for r in rows]
    assert all(_doc_config(d)["a"] == _doc_config(d)["b"] for d in docs)
    # keep: rows with a == 1 are never suggested
    kept = tpe.suggest_sampled(ids, domain, trials, SEED, draw="joint",
                               keep=lambda cols: cols["a"] != 1, **kw)
    a = pool.vals[:, list(domain.params).index("a")]
    want = _expected_order(S, (a == 1).astype(np.uint8), len(ids))
    assert (a == 1).any() and [_doc_config(d) for d in kept] == [pool.config(int(r)) for r in want]
    # distinct: every configuration is in the history -> nothing is fresh
    assert tpe.suggest_sampled(ids, domain, trials, SEED, draw="joint", distinct=True, **kw) == []
    # a history without three configurations: those, once each, and nothing else
    domain2, trials2 = _diagonal(drop={3, 5, 10})
    fresh = tpe.suggest_sampled(ids, domain2, trials2, SEED, draw="joint", distinct=True, **kw)
    got = sorted(4 * _doc_config(d)["a"] + _doc_config(d)["b"] for d in fresh)
    assert got == [3, 5, 10]
    # the startup phase is today's
    start = dict(n_EI_candidates=64, n_startup_jobs=65, verbose=False)
    d1 = tpe.suggest_sampled(ids, domain, trials, 9, joint=True, draw="joint", **start)
    d2 = tpe.suggest_sampled(ids, domain, trials, 9, **start)
    assert [d["misc"]["vals"] for d in d1] == [d["misc"]["vals"] for d in d2]


def test_draw_factorised_is_the_call_without_draw():
    domain, trials, _ = _all_kinds()
    ids = [700, 701, 702, 703, 704]
    kw = dict(n_EI_candidates=256, joint=True, bandwidth=KW["bandwidth"],
              cat_smoothing=KW["cat_smoothing"], verbose=False,
              **{k: KW[k] for k in ("prior_weight", "gamma", "linear_forgetting")})
    today = tpe.suggest_sampled(ids, domain, trials, 123, **kw)
    named = tpe.suggest_sampled(ids, domain, trials, 123, draw="factorised", **kw)
    assert [d["misc"] for d in named] == [d["misc"] for d in today]
    drawn = tpe.suggest_sampled(ids, domain, trials, 123, draw="joint", **kw)
    assert [d["misc"]["vals"] for d in drawn] != [d["misc"]["vals"] for d in today]


def test_fmin_on_the_diagonal_objective():
    space = U.diagonal_case(hp)[0]
    trials = Trials()
    algo = partial(tpe.suggest_sampled, n_EI_candidates=256, gamma=2.0, joint=True, draw="joint",
                   verbose=False)
    fmin(lambda cfg: float(cfg["a"] != cfg["b"]), space, algo=algo, max_evals=40,
         max_queue_len=4, trials=trials, rstate=np.random.RandomState(0), show_progressbar=False)
    assert len(trials) == 40


def test_a_space_without_a_joint_label_raises():
    empty = Domain(lambda x: 0, {"x": 1.0})
    none = U.make_trials(empty, [{}] * 3, [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="joint"):
        tpe.Pool.sample(empty, none, 0, 16, joint=True)
    with pytest.raises(ValueError, match="joint"):
        tpe.suggest_sampled([1], empty, none, 0, n_startup_jobs=0, joint=True, draw="joint",
                            verbose=False)


# -- 5. limits -----------------------------------------------------------------------------
def test_limits_are_unsupported_and_bad_arguments_are_refused():
    lib = L.load()
    rec = np.zeros(L.COND_MAX_LABELS + 1, L.JOINT_LABEL_DTYPE)
    rec["kind"], rec["prior_sigma"], rec["prior_r"] = L.JOINT_CONT, 1.0, 1.0
    host = rec.ctypes.data

    def call(h, D, n=4, n_cat_cdf=0, one_plus_a=2.0, row_base=0, n_rows=16, ld=16, n_cols=1024):
        return lib.tpe_joint_sample(h, None, D, None, n, None, None, n_cat_cdf, None, one_plus_a,
                                    row_base, n_rows, None, ld, n_cols, None, None)
    assert call(host, L.COND_MAX_LABELS + 1) == L.E_UNSUPPORTED
    cat = np.zeros(1, L.JOINT_LABEL_DTYPE)
    cat["kind"], cat["n_cat"] = L.JOINT_CAT, L.JOINT_MAX_CAT + 1
    assert call(cat.ctypes.data, 1) == L.E_UNSUPPORTED
    cat["n_cat"] = 4  # fits, but its cdf does not: refused before any launch
    assert call(cat.ctypes.data, 1, n_cat_cdf=3) == -1
    cat["tab_off"] = 4  # not a label's place in the tables
    assert call(cat.ctypes.data, 1, n_cat_cdf=64) == -1
    assert call(host, 0) == -1                         # no label
    assert call(host, 1) == -1                         # null pointers
    assert call(host, 1, n=-1) == -1
    assert call(host, 1, n_rows=17) == -1              # more rows than the block holds
    assert call(host, 1, row_base=-1) == -1
    assert call(host, 1, one_plus_a=0.5) == -1
    assert call(host, 1, one_plus_a=float("nan")) == -1
    assert b"tpe_joint_sample" in lib.tpe_last_error()
    assert call(host, 1, n_rows=0) == 0                # nothing to draw: a no-op
    rec["col"][0] = 4096                               # a column the block lacks
    assert call(host, 1) == -1
