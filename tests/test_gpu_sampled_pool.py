"""A pool sampled from the posterior: the kernels of csrc/tpe_sampled.hip
alone, Pool.sample against the engine's own per-candidate outputs, and
tpe.suggest_sampled.

Reference of the born values and terms: ``Engine.run(..., precision=64,
outputs=True)`` of the same works.  For a drawn quantized label that call
scores the value lattice and keeps nothing per candidate, so there the
reference is the sampler hook (``sample_only=True``: the label's stream) and
the exact scores of those values injected.
"""
import ctypes
from dataclasses import replace
from functools import partial

import numpy as np
import pytest

from hyperopt_amd import Domain, Trials, fmin, hp, rand, tpe
from hyperopt_amd import _lib as L
from hyperopt_amd import pool as pool_mod
from hyperopt_amd.walk import int_offset
from oracle import tpe_oracle as O
from tests import cond_util as C
from tests.golden import spaces
from tests.test_gpu_pool import _case, _expected_order, _fold_numpy, _same_bits

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 257, 4097]
INT_KINDS = ("randint", "categorical")


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _space(name):
    maker = spaces.SPACES.get(name) or C.CRAFTED[name]
    return Domain(lambda x: 0, maker(hp))


# -- 1. tpe_rows_active alone ---------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("space", ["nested", "shared_node"])
def test_rows_active(space, n):
    import torch
    domain = _space(space)
    lo, co, terms = pool_mod.program_csr(domain)
    nl, ld = len(domain.params), n + 37
    cols = C.random_columns(domain, n, np.random.RandomState(n), ld=ld)
    d_vals = _up(cols)
    d_act = torch.full((nl, ld), 7, dtype=torch.uint8, device=_dev())  # poisoned padding
    d_n = torch.zeros(nl, dtype=torch.int64, device=_dev())
    L.check(L.load().tpe_rows_active(d_vals.data_ptr(), ld, n, nl, lo.ctypes.data, co.ctypes.data,
                                     terms.ctypes.data, len(terms), d_act.data_ptr(),
                                     d_n.data_ptr(), _stream()), "tpe_rows_active")
    act = d_act.cpu().numpy()
    want = C.interpret(lo, co, terms, cols, n)
    np.testing.assert_array_equal(act[:, :n], want.astype(np.uint8))
    assert (act[:, n:] == 7).all()
    np.testing.assert_array_equal(d_n.cpu().numpy(), want.sum(1))


# -- 2. tpe_pool_ranges alone ---------------------------------------------------
def _extrema(sel):
    """numpy's min / max of ``sel`` with -0.0 ordered below +0.0 (numpy's own
    pick between the two zeros depends on their order in the array)."""
    if not sel.size:
        return np.inf, -np.inf
    lo, hi = sel.min(), sel.max()
    zeros = sel[sel == 0]
    if lo == 0:
        lo = -0.0 if np.signbit(zeros).any() else 0.0
    if hi == 0:
        hi = 0.0 if (~np.signbit(zeros)).any() else -0.0
    return lo, hi


@pytest.mark.parametrize("n", ROWS)
def test_pool_ranges(n):
    import torch
    rng = np.random.RandomState(100 + n)
    nl, ld = 7, n + 11
    vals = rng.normal(size=(nl, ld)) * 10
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -3.5, 0.0, 1e-300, -1e-300])
    where = rng.rand(nl, ld) < 0.3
    vals[where] = special[rng.randint(0, special.size, int(where.sum()))]
    active = rng.rand(nl, ld) < 0.6
    active[2] = False                                  # live in no row
    vals[3] = np.where(rng.rand(ld) < 0.5, np.nan, np.inf)  # no finite live value
    vals[4] = np.where(rng.rand(ld) < 0.5, 0.0, -0.0)       # zeros of both signs only
    vals[5] = -np.abs(vals[5])                              # nothing > 0
    d_vals, d_act = _up(vals), _up(active.view(np.uint8))
    for positive in (0, 1):
        flags = np.full(nl, positive, np.uint8)
        d_out = torch.full((2 * nl,), 7.0, dtype=torch.float64, device=_dev())
        L.check(L.load().tpe_pool_ranges(d_vals.data_ptr(), d_act.data_ptr(), ld, n, nl,
                                         flags.ctypes.data, d_out.data_ptr(), _stream()),
                "tpe_pool_ranges")
        got = d_out.cpu().numpy().reshape(nl, 2)
        for j in range(nl):
            sel = vals[j, :n][active[j, :n]]
            sel = sel[np.isfinite(sel)]
            if positive:
                sel = sel[sel > 0]
            assert _same_bits(got[j], np.asarray(_extrema(sel))), (n, positive, j, got[j])


# -- 3. tpe_pool_take alone -----------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 64])
def test_pool_take(k):
    import torch
    rng = np.random.RandomState(k)
    nl, n, ld = 7, 300, 311
    vals = rng.normal(size=(nl, ld))
    active = rng.rand(nl, ld) < 0.5
    rows = rng.randint(0, n, k)  # arbitrary order, with repeats from k = 64 on
    if k > 1:
        rows[1] = rows[0]
    d_vals, d_act, d_rows = _up(vals), _up(active.view(np.uint8)), _up(rows.astype(np.int64))
    d_ov = torch.empty((k, nl), dtype=torch.float64, device=_dev())
    d_oa = torch.empty((k, nl), dtype=torch.uint8, device=_dev())
    L.check(L.load().tpe_pool_take(d_vals.data_ptr(), d_act.data_ptr(), ld, nl, d_rows.data_ptr(),
                                   k, d_ov.data_ptr(), d_oa.data_ptr(), _stream()),
            "tpe_pool_take")
    assert _same_bits(d_ov.cpu().numpy(), vals[:, rows].T)
    np.testing.assert_array_equal(d_oa.cpu().numpy(), active[:, rows].T.astype(np.uint8))


# -- 4. Pool.sample -------------------------------------------------------------
SEED = 1234


def _reference(domain, trials, meta, n):
    """(cand, bl, al), each (L, n): the engine's own per-candidate outputs of
    the works Pool.sample names (module doc for the quantized labels)."""
    labels = list(domain.params)
    eng, obs = pool_mod._history_inputs(domain, trials, meta["gamma"])
    kw = dict(prior_weight=meta["prior_weight"], lf=25, precision=64)
    works = [obs.work(lab, domain.specs[lab], j, n_cand=n, n_total=n,
                      key=tpe.label_key(SEED, lab), cand_base=0) for j, lab in enumerate(labels)]
    res = eng.run(works, outputs=True, **kw, **obs.run_kwargs)
    cand = np.stack([r.cand for r in res])
    bl = np.stack([r.below_llik for r in res])
    al = np.stack([r.above_llik for r in res])
    quant = [j for j, lab in enumerate(labels) if domain.specs[lab].kind.startswith("q")]
    if quant:
        drawn = eng.run([works[j] for j in quant], sample_only=True, **kw, **obs.run_kwargs)
        inj = eng.run([replace(works[j], cand=r.cand.copy(), n_cand=n)
                       for j, r in zip(quant, drawn)], outputs=True, **kw, **obs.run_kwargs)
        for j, r, s in zip(quant, drawn, inj):
            cand[j], bl[j], al[j] = r.cand, s.below_llik, s.above_llik
    return cand, bl, al


@pytest.mark.parametrize("n", [1, 65, 4097])
@pytest.mark.parametrize("case", ["nested", "readme", "many_dists"])
def test_pool_sample(case, n, monkeypatch):
    arrays, meta, trials, domain = _case(case)
    labels = list(domain.params)
    nl = len(labels)
    kw = dict(prior_weight=meta["prior_weight"], gamma=meta["gamma"])
    cand, bl, al = _reference(domain, trials, meta, n)
    pool = tpe.Pool.sample(domain, trials, SEED, n, keep_terms=True, **kw)
    assert isinstance(pool, tpe.Pool) and len(pool) == n and pool.n_untaken == n
    S, terms = pool.scores(), pool.terms()
    dv = pool._born().vals[:, :n].cpu().numpy()
    # 1. values: candidate r of every label's stream, offset-free on the device
    for j, lab in enumerate(labels):
        assert _same_bits(dv[j], cand[j]), lab
    vals, active = pool.vals, pool.active
    assert vals.shape == active.shape == (n, nl)
    for j, lab in enumerate(labels):
        off = int_offset(domain.specs[lab]) or 0
        a = active[:, j]
        assert _same_bits(vals[a, j], cand[j][a] + off if off else cand[j][a]), lab  # (-0.0 stays)
        assert np.isnan(vals[~a, j]).all()
    # 2. terms: the draws' own log l - log g where live, NaN where not
    with np.errstate(invalid="ignore"):
        t_ref = (bl - al).T
    np.testing.assert_array_equal(np.isnan(terms), ~active)
    assert _same_bits(terms[active], t_ref[active])
    # 3. activity: the program on the pool's own selector columns
    lo, co, tm = pool_mod.program_csr(domain)
    np.testing.assert_array_equal(active.T, C.interpret(lo, co, tm, dv, n))
    np.testing.assert_array_equal(pool.n_active, active.sum(0))
    plain = tpe.Pool.from_arrays(domain, vals, active)  # validates
    # 4. the fold's bits; label chunks change nothing
    assert _same_bits(S, _fold_numpy(terms, active))
    monkeypatch.setattr(pool_mod, "CHUNK_ELEMS", 2 * n)
    pool2 = tpe.Pool.sample(domain, trials, SEED, n, keep_terms=True, **kw)
    assert _same_bits(pool2._born().vals[:, :n].cpu().numpy(), dv)
    assert _same_bits(pool2.scores(), S) and _same_bits(pool2.terms()[active], terms[active])
    np.testing.assert_array_equal(pool2.active, active)
    monkeypatch.undo()
    # 5. the same rows scored again as injected candidates: the pool tolerance
    with np.errstate(invalid="ignore"):
        scale = np.where(active, np.abs(bl.T) + np.abs(al.T), 0.0).sum(1)
    S2 = tpe.score_configs(domain, trials, plain, **kw)
    err = np.abs(S2 - S)
    print(case, n, "max |S_rescored - S_born| = %.3g" % err.max())
    assert (err <= 1e-6 * scale).all()
    S3 = tpe.score_configs(domain, trials, pool, **kw)  # the born pool's own columns
    assert (np.abs(S3 - S) <= 1e-6 * scale).all()
    # 6. the ranges a re-score names, computed on the device
    ranges = pool._born().ranges
    assert ranges is not None and len(ranges) == nl
    for j, lab in enumerate(labels):
        spec = domain.specs[lab]
        live = (vals[:, j] - (int_offset(spec) or 0))[active[:, j]]
        assert tuple(ranges[j]) == tuple(pool_mod._scoring_range(spec, live)), lab
    # 7. the oracle
    if case == "nested":
        for j, lab in enumerate(labels):
            spec = domain.specs[lab]
            below, above = O.ap_split_trials(arrays["obs_idxs/" + lab], arrays["obs_vals/" + lab],
                                             arrays["hist_tids"], arrays["hist_losses"],
                                             meta["gamma"])
            a = active[:, j]
            fn = O.categorical_label_scores if spec.kind in INT_KINDS else \
                O.continuous_label_scores
            with np.errstate(all="ignore"):
                ref = fn(spec.kind, spec.args, below, above, vals[a, j],
                         prior_weight=meta["prior_weight"])
            rb, ra = ref["below_llik"], ref["above_llik"]
            e = np.abs(terms[a, j] - (rb - ra))
            assert (e <= 1e-6 * (np.abs(rb) + np.abs(ra))).all(), (lab, e.max() if e.size else 0)


def test_pool_sample_empty_and_marks():
    arrays, meta, trials, domain = _case("nested")
    empty = tpe.Pool.sample(domain, trials, SEED, 0)
    assert len(empty) == 0 and empty.n_untaken == 0
    pool = tpe.Pool.sample(domain, trials, SEED, 300, prior_weight=meta["prior_weight"],
                           gamma=meta["gamma"])
    S = pool.scores()
    pool.mark_taken([3, 5])
    pool.release([5])
    assert pool.n_untaken == 299
    docs = tpe.suggest_from_pool([900, 901, 902], domain, trials, 0, pool=pool,
                                 prior_weight=meta["prior_weight"], gamma=meta["gamma"],
                                 n_startup_jobs=1)
    S2 = pool.scores()  # the same history: the re-scored S, within the last bits of the born one
    taken = np.zeros(300, np.uint8)
    taken[3] = 1
    rows = [pool.row_of[t] for t in (900, 901, 902)]
    assert rows == list(_expected_order(S2, taken, 3))
    assert np.abs(S2 - S).max() < 1e-6 * max(1.0, np.abs(S).max())
    for d, r in zip(docs, rows):
        assert {k: v[0] for k, v in d["misc"]["vals"].items() if v} == pool.config(r)


# -- 5. tpe.suggest_sampled -------------------------------------------------------
def _doc_config(doc):
    return {k: v[0] for k, v in doc["misc"]["vals"].items() if v}


def _row_config(domain, pool, r):
    cfg = pool.config(int(r))
    for lab, v in cfg.items():
        assert isinstance(v, int) == (domain.specs[lab].kind in INT_KINDS), lab
    return cfg


def test_suggest_sampled_order_seeds_keep():
    arrays, meta, trials, domain = _case("nested")
    kw = dict(prior_weight=meta["prior_weight"], gamma=meta["gamma"])
    args = dict(n_EI_candidates=300, n_startup_jobs=1, **kw)
    ids = [700, 701, 702, 703, 704]
    pool = tpe.Pool.sample(domain, trials, 42, 300, **kw)
    S = pool.scores()
    docs = tpe.suggest_sampled(ids, domain, trials, 42, **args)
    rows = _expected_order(S, np.zeros(300), 5)
    assert [d["tid"] for d in docs] == ids
    assert [_doc_config(d) for d in docs] == [_row_config(domain, pool, r) for r in rows]
    for d in docs:  # exactly the live labels
        live = set(domain.reachable({k: v for k, v in _doc_config(d).items()}))
        assert {k for k, v in d["misc"]["vals"].items() if v} == live
    again = tpe.suggest_sampled(ids, domain, trials, 42, **args)
    assert [_doc_config(d) for d in again] == [_doc_config(d) for d in docs]
    other = tpe.suggest_sampled(ids, domain, trials, 43, **args)
    assert [_doc_config(d) for d in other] != [_doc_config(d) for d in docs]
    # keep: rows whose root is 1 are never suggested
    seen = []

    def keep(cols):
        seen.append(len(cols["root"]))
        assert set(cols) == set(domain.params)
        return cols["root"] != 1
    kept = tpe.suggest_sampled(ids, domain, trials, 42, keep=keep, **args)
    root = pool.vals[:, list(domain.params).index("root")]
    assert (root == 1).any() and (root != 1).any() and seen == [300]
    want = _expected_order(S, (root == 1).astype(np.uint8), 5)
    assert [_doc_config(d) for d in kept] == [_row_config(domain, pool, r) for r in want]
    assert all(_doc_config(d)["root"] != 1 for d in kept)
    with pytest.raises(ValueError):
        tpe.suggest_sampled(ids, domain, trials, 42, keep=lambda cols: np.ones(3, bool), **args)
    assert tpe.suggest_sampled(ids, domain, trials, 42,
                               keep=lambda cols: np.zeros(len(cols["root"]), bool), **args) == []
    # more ids than rows
    few = tpe.suggest_sampled(ids, domain, trials, 42, **dict(args, n_EI_candidates=3))
    assert [d["tid"] for d in few] == ids[:3]
    assert tpe.suggest_sampled(ids, domain, trials, 42, **dict(args, n_EI_candidates=0)) == []


def test_suggest_sampled_startup():
    arrays, meta, trials, domain = _case("nested")
    ids = [800, 801, 802]
    T = len(trials.trials)
    docs = tpe.suggest_sampled(ids, domain, trials, 9, n_startup_jobs=T + 1)
    want = rand.suggest_device(ids, domain, trials, 9)
    assert [_doc_config(d) for d in docs] == [_doc_config(d) for d in want]
    labels, draws = rand.draw_priors(domain, 9, 64)
    root = draws[labels.index("root")]
    kept = tpe.suggest_sampled(ids, domain, trials, 9, n_EI_candidates=64, n_startup_jobs=T + 1,
                               keep=lambda cols: cols["root"] == 2)
    first = np.flatnonzero(root == 2)[:3]
    assert len(kept) == len(first) == 3
    configs = rand._configs(domain, labels, draws[:, first])
    assert [_doc_config(d) for d in kept] == configs


def test_suggest_sampled_host_fallback():
    """A switch on an expression of labels: no program, the activity comes
    from ``reachable`` on the host."""
    domain = _space("expr_selector")
    assert domain.live_program() is None
    trials = Trials()
    fmin(lambda x: 0.0, C.expr_selector(hp), algo=rand.suggest, max_evals=30, trials=trials,
         rstate=np.random.RandomState(3), show_progressbar=False)
    labels = list(domain.params)
    pool = tpe.Pool.sample(domain, trials, 5, 257)
    vals, active = pool.vals, pool.active
    for r in range(257):
        decided = {lab: int(vals[r, labels.index(lab)]) for lab in ("a", "b")}
        assert {labels[j] for j in np.flatnonzero(active[r])} == set(domain.reachable(decided)), r
    np.testing.assert_array_equal(pool.n_active, active.sum(0))
    tpe.Pool.from_arrays(domain, vals, active)  # validates
    docs = tpe.suggest_sampled([50, 51], domain, trials, 5, n_EI_candidates=257)
    rows = _expected_order(pool.scores(), np.zeros(257), 2)
    assert [_doc_config(d) for d in docs] == [pool.config(int(r)) for r in rows]


def test_fmin_with_suggest_sampled():
    calls = []

    def algo(new_ids, domain, trials, seed):
        docs = tpe.suggest_sampled(new_ids, domain, trials, seed, n_EI_candidates=256)
        calls.append((len(trials.trials), len(new_ids), docs))
        return docs

    def fn(cfg):
        return {"lin": 1.0, "tree": 0.5, "nn": 0.2}[cfg["kind"]] + 0.01 * len(str(cfg))
    trials = Trials()
    fmin(fn, spaces.nested(hp), algo=algo, max_evals=40, max_queue_len=4, trials=trials,
         rstate=np.random.RandomState(0), show_progressbar=False)
    assert len(trials) == 40
    late = [(n_ids, docs) for T, n_ids, docs in calls if T >= 20 and n_ids == 4]
    assert late
    for n_ids, docs in late:
        assert len(docs) == 4
        assert len({tuple(sorted(_doc_config(d).items())) for d in docs}) == 4
    trials2 = Trials()
    fmin(fn, spaces.nested(hp), algo=partial(tpe.suggest_sampled, n_EI_candidates=256),
         max_evals=40, max_queue_len=4, trials=trials2, rstate=np.random.RandomState(0),
         show_progressbar=False)
    assert len(trials2) == 40
