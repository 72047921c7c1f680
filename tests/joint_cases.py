"""The case table of the joint Parzen kernels' stage tests (csrc/tpe_joint.hip).

Shared by tests/test_joint_cases.py (CPU: the premises) and
tests/test_gpu_joint_stages.py (GPU: the kernels).  ``build_inputs()`` makes
every case's inputs from fixed seeds; tests/golden/make_joint_cases.py adds
the expected values, computed with mpmath at 50 digits, and writes
tests/golden/joint_cases.npz; ``load()`` reads that file, inputs included, so
the tests have one source of truth.

A case is a dict:

  labels   records of ``_lib.JOINT_LABEL_DTYPE`` as the C entry points take them
           (``tab_off`` and ``prior_r`` filled as joint._device_labels fills them)
  probs    the discrete labels' prior probabilities, concatenated in label order
  hist     (N, n_cols) history values as the history stores them (randint with
           its ``low``); NaN in the columns no label uses
  sets     row lists (int32): set s is the mixture of hist[sets[s]] + the prior
  sig      (n_sets, D) the trial components' sigma (joint.bandwidths' expression)
  pool     (P, n_cols) pool values as the device pool stores them (randint
           without its ``low``)
  lf, prior_weight, bandwidth, smoothing
  onehot   component indices whose a_i alone is in the fixture (set 0)

and, from the fixture, per set s: ``logl`` (P,), ``cond`` (P,); per one-hot
index: ``a`` (P,), ``cond`` (P,).

The tolerance of every comparison is K * 2**-53 * cond: ``cond`` (the module
text of make_joint_cases.py) is the first-order bound of one rounding per
operation, K_CPU is what glibc's libm needs against the 50-digit values
(measured and asserted in test_joint_cases.py), and the device gets K_DEV = 8
K_CPU rounded up to a power of two, for its four known differences: a multiply
by 1 / (sqrt(2) sigma) where numpy divides, an fma for -u^2, ROCm's erf / exp /
log, and the clamp of sqrt(2) sigma at 1e-12.
"""
import json
import math
import os

import numpy as np

from hyperopt_amd import _lib as L

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "joint_cases.npz")
P = 40
EPS = 1e-12
U53 = 2.0 ** -53
# the largest |score_numpy - fixture| / (2**-53 cond) over every case and set, as
# test_joint_cases.py measures it (1.727, on labels128: 128 factors per
# component), rounded up to a power of two because glibc picks its exp / log
# variant by CPU; the test asserts K_CPU / 2 < measured <= K_CPU.  The device
# gets 8 times that (8 x 1.727 rounded up to a power of two is the same 16).
K_CPU = 2.0
K_DEV = 16.0
GEO_C = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 255, 256, 257, 264, 265, 512, 513)
ONEHOT_C = (9, 257, 265, 513)
LABEL_COUNTS = (1, 32, 33, 128)
PREP_N = (0, 7, 8, 255, 256)
PUBLIC = {"pub257": (261, (3, 50, 100, 150, 200)), "pub513": (518, (3, 50, 100, 150, 200, 400))}


# -- label kinds -------------------------------------------------------------------
def _spec(kind, log=False, bounded=False, lo=0.0, hi=0.0, q=0.0, mu=0.0, sigma=0.0, p=None,
          shift=0):
    return dict(kind=kind, log=log, bounded=bounded, lo=float(lo), hi=float(hi), q=float(q),
                mu=float(mu), sigma=float(sigma), p=None if p is None else np.asarray(p, float),
                shift=int(shift))


def uniform(lo, hi):
    return _spec(L.JOINT_CONT, bounded=True, lo=lo, hi=hi, mu=0.5 * (lo + hi), sigma=hi - lo)


def loguniform(lo, hi):
    return dict(uniform(lo, hi), log=True)


def normal(mu, sigma):
    return _spec(L.JOINT_CONT, mu=mu, sigma=sigma)


def lognormal(mu, sigma):
    return dict(normal(mu, sigma), log=True)


def quniform(lo, hi, q):
    return dict(uniform(lo, hi), kind=L.JOINT_QUANT, q=float(q))


def qloguniform(lo, hi, q):
    return dict(quniform(lo, hi, q), log=True)


def qnormal(mu, sigma, q):
    return dict(normal(mu, sigma), kind=L.JOINT_QUANT, q=float(q))


def qlognormal(mu, sigma, q):
    return dict(qnormal(mu, sigma, q), log=True)


def cat(p, shift=0):
    return _spec(L.JOINT_CAT, p=p, shift=shift)


def records(specs, cols):
    """(label records, concatenated probabilities) of ``specs`` on columns ``cols``."""
    rec = np.zeros(len(specs), L.JOINT_LABEL_DTYPE)
    probs, off = [], 0
    for d, (s, col) in enumerate(zip(specs, cols)):
        r = rec[d]
        r["kind"], r["col"] = s["kind"], col
        r["flags"] = (L.JOINT_LOG if s["log"] else 0) | (L.JOINT_BOUNDED if s["bounded"] else 0)
        r["lo"], r["hi"], r["q"] = s["lo"], s["hi"], s["q"]
        r["prior_mu"], r["prior_sigma"], r["shift"] = s["mu"], s["sigma"], s["shift"]
        if s["kind"] == L.JOINT_CAT:
            r["n_cat"], r["tab_off"] = s["p"].size, off
            probs.append(s["p"])
            off += 3 * s["p"].size
        else:
            r["prior_r"] = 1.0 / (math.sqrt(2.0) * s["sigma"])
    return rec, (np.concatenate(probs) if probs else np.zeros(0))


def label_probs(case, d):
    """The prior probabilities of discrete label d."""
    lab = case["labels"]
    off = int(lab["tab_off"][d]) // 3
    return case["probs"][off:off + int(lab["n_cat"][d])]


def bandwidths(labels, n, bandwidth):
    """joint.bandwidths' expression on label records."""
    D = len(labels)
    scale = float(bandwidth) * float(n) ** (-1.0 / (D + 4)) if n else 0.0
    return np.asarray([scale * float(s) for s in labels["prior_sigma"]])


def _case(name, specs, cols, n_cols, hist, sets, pool, lf=25, prior_weight=0.7, bandwidth=1.0,
          smoothing=1.0, onehot=(), losses=None):
    labels, probs = records(specs, cols)
    sets = [np.asarray(s, np.int32) for s in sets]
    case = dict(name=name, labels=labels, probs=probs,
                hist=np.ascontiguousarray(hist, np.float64), sets=sets,
                sig=np.stack([bandwidths(labels, s.size, bandwidth) for s in sets]),
                pool=np.ascontiguousarray(pool, np.float64), lf=int(lf),
                prior_weight=float(prior_weight), bandwidth=float(bandwidth),
                smoothing=float(smoothing), onehot=np.asarray(onehot, np.int64))
    assert case["hist"].shape[1] == n_cols and case["pool"].shape == (P, n_cols)
    if losses is not None:
        case["losses"] = np.asarray(losses, np.float64)
    return case


# -- the cases ---------------------------------------------------------------------
GEO_PCHOICE = (0.1, 0.2, 0.3, 0.4)


def geo_specs():
    return [loguniform(-2, 2), quniform(0, 10, 1), cat(GEO_PCHOICE)]


def _geo_arrays():
    rng = np.random.RandomState(20240)
    N = 518
    hist = np.stack([np.exp(rng.uniform(-2, 2, N)), np.rint(rng.uniform(0, 10, N)),
                     rng.randint(0, 4, N).astype(float)], 1)
    pool = np.stack([np.exp(np.linspace(-2, 2, P))[rng.permutation(P)],
                     (np.arange(P) % 11).astype(float), (np.arange(P) // 3 % 4).astype(float)], 1)
    return hist, pool, rng.permutation(512)


def onehot_indices(C):
    want = [0, 7, 8, C - 2, C - 1, 255, 256, 257]
    return sorted({i for i in want if 0 <= i < C})


def _geometry():
    hist, pool, perm = _geo_arrays()
    out = []
    for C in GEO_C:
        out.append(_case("geo%d" % C, geo_specs(), (0, 1, 2), 3, hist, [perm[:C - 1]], pool,
                         onehot=onehot_indices(C) if C in ONEHOT_C else ()))
    # the same space as real Trials: the above set the rows the split leaves
    for name, (N, below) in PUBLIC.items():
        losses = 1.0 + 1e-3 * np.arange(N)
        losses[list(below)] = 1e-3 * np.arange(len(below))
        above = [r for r in range(N) if r not in below]
        out.append(_case(name, geo_specs(), (0, 1, 2), 3, hist[:N], [list(below), above], pool,
                         losses=losses))
    return out


def _running():
    """One normal label, C = 513, a_i spanning more than 800 on every row."""
    i = np.arange(512)
    x = (12.6 + 1.4 * np.arange(P) / (P - 1))[:, None]
    mus = {"run_up": (12.0 * i / 511, 12.5), "run_down": (12.0 * (511 - i) / 511, -0.5),
           "run_mid": (12.0 - 12.0 * np.abs(i - 384) / 384, -0.5)}
    return [_case(name, [normal(pm, 1.0)], (0,), 1, mu[:, None], [i], x, lf=1000)
            for name, (mu, pm) in mus.items()]


def _dead():
    """One qnormal label, C = 513: whole chunks (dead_chunks) and runs of passes
    inside a chunk (dead_passes) whose every component has mass 0 for a row."""
    i = np.arange(512)
    near = (i % 3 - 1).astype(float)
    r = np.arange(P)
    # rows 0..14 at the far cluster (chunk 0 dead, chunk 1 finite, the prior
    # dead), 15..29 at the near one (the reverse; the prior finite), 30..39
    # far from both (every chunk dead)
    x = np.where(r < 15, 1000.0 + r % 3 - 1, np.where(r < 30, r % 3 - 1.0, 5000.0 + r))
    specs = [qnormal(0.0, 2.0, 1.0)]
    chunks = near + 1000.0 * (i >= 256)
    passes = near + 1000.0 * ((i // 64) % 2 == 0)  # (chunk 0 starts dead for a near row)
    return [_case("dead_chunks", specs, (0,), 1, chunks[:, None], [i], x[:, None]),
            _case("dead_passes", specs, (0,), 1, passes[:, None], [i], x[:, None])]


def _edges():
    rng = np.random.RandomState(777)
    N = 20
    first = np.exp(rng.uniform(-2, 2, N))
    cats = rng.randint(1, 3, N).astype(float)
    sets = [[1, 4, 9, 13, 17], [0, 2, 3, 5, 6, 7, 8, 10, 11, 12, 14, 15]]
    px = np.exp(rng.uniform(-2, 2, P))
    pc = (np.arange(P) % 2 + 1).astype(float)
    pch = cat((0.0, 0.4, 0.6))
    out = []

    def add(name, specs, h1, p1, h0=first, p0=px, hc=cats, pcat=pc):
        out.append(_case(name, specs, (0, 1, 2), 3, np.stack([h0, h1, hc], 1), sets,
                         np.stack([p0, p1, pcat], 1)))

    # qlognormal(0, 1, 1): x = 0 (the lower edge <= 0: Phi_l = 0), x = q, and a
    # row far out (-inf under every component); an observation of 0 in set 1
    h = (1.0 + np.arange(N) % 4)
    h[7] = 0.0
    p = (np.arange(P) % 6).astype(float)
    p[5] = 1.0e9
    add("edge_qlognormal", [loguniform(-2, 2), qlognormal(0, 1, 1), pch], h, p)
    # qloguniform(0, 3, 2): x = 0 clips both edges to lo (mass 0), x = 20 clips
    # the upper one to hi
    h = 2.0 + 2.0 * (np.arange(N) % 10)
    p = 2.0 * (np.arange(P) % 11)
    add("edge_qloguniform", [loguniform(-2, 2), qloguniform(0, 3, 2), pch], h, p)
    # quniform(0, 10, 3): x = 0 and x = 9 have an edge clipped at lo / hi; at
    # x = -1.5 the upper edge lands exactly on lo
    h = 3.0 * (np.arange(N) % 4)
    p = 3.0 * (np.arange(P) % 4)
    p[[6, 21]] = -1.5
    add("edge_quniform", [loguniform(-2, 2), quniform(0, 10, 3), pch], h, p)
    # lognormal at x = 0.0: t = log 1e-12
    p0 = px.copy()
    p0[[2, 30]] = 0.0
    add("edge_lognormal", [lognormal(0, 1), quniform(0, 10, 3), pch], h, 3.0 * (np.arange(P) % 4),
        p0=p0)
    # the pchoice option of probability 0 in pool rows: set 0 has a component
    # of that category (row 9 of the history), set 1 has none
    hc = cats.copy()
    hc[9] = 0.0
    pcat = pc.copy()
    pcat[[0, 11, 33]] = 0.0
    add("edge_pchoice", [loguniform(-2, 2), quniform(0, 10, 1), pch],
        np.rint(rng.uniform(0, 10, N)), (np.arange(P) % 11).astype(float), hc=hc, pcat=pcat)
    return out


def all_kind_specs():
    """The eleven kinds the label-count and the prep cases cycle through."""
    return [uniform(4, 7), loguniform(-2, 0), quniform(0, 10, 3), qloguniform(0, 3, 2),
            normal(4, 7), lognormal(-2, 2), qnormal(0, 10, 2), qlognormal(0, 2, 1),
            cat([0.2] * 5), cat([1.0 / 13] * 13, shift=12), cat((0.0, 0.4, 0.6))]


def _draw(spec, rng, n, stored):
    """n values inside the support of ``spec``; ``stored``: as a history holds
    them (with randint's low)."""
    u = rng.uniform(size=n)
    if spec["kind"] == L.JOINT_CAT:
        K = spec["p"].size
        c = np.where(spec["p"][0] == 0.0, 1 + np.floor(u * (K - 1)), np.floor(u * K))
        return c + (spec["shift"] if stored else 0)
    if spec["bounded"]:
        v = spec["lo"] + u * (spec["hi"] - spec["lo"])
    else:
        v = spec["mu"] + (2.0 * u - 1.0) * spec["sigma"]
    if spec["log"]:
        v = np.exp(v)
    if spec["q"]:
        v = np.rint(v / spec["q"]) * spec["q"]
        if spec["log"]:
            v = np.maximum(v, spec["q"])
    return v


def _label_counts():
    out = []
    kinds = all_kind_specs()
    for D in LABEL_COUNTS:
        rng = np.random.RandomState(500 + D)
        n_cols = D + 3
        specs = [kinds[d % len(kinds)] for d in range(D)]
        cols = rng.permutation(n_cols)[:D]
        hist, pool = np.full((8, n_cols), np.nan), np.full((P, n_cols), np.nan)
        for s, c in zip(specs, cols):
            hist[:, c], pool[:, c] = _draw(s, rng, 8, True), _draw(s, rng, P, False)
        out.append(_case("labels%d" % D, specs, cols, n_cols, hist, [rng.permutation(8)], pool))
    return out


def _prep():
    """The history the prep read-back uses: every kind, 300 rows, values of 0.0
    and 1e-13 on the unbounded log kinds; set s has the first PREP_N[s] rows of
    a permutation."""
    rng = np.random.RandomState(901)
    specs = all_kind_specs()
    D, N = len(specs), 300
    cols = rng.permutation(D + 2)[:D]
    hist, pool = np.full((N, D + 2), np.nan), np.full((P, D + 2), np.nan)
    for s, c in zip(specs, cols):
        hist[:, c], pool[:, c] = _draw(s, rng, N, True), _draw(s, rng, P, False)
    perm = rng.permutation(N)
    hist[perm[[0, 3, 200]], cols[5]] = [0.0, 1e-13, 0.0]   # lognormal
    hist[perm[[1, 6, 255]], cols[7]] = 0.0                 # qlognormal
    return _case("prep", specs, cols, D + 2, hist, [perm[:n] for n in PREP_N], pool)


def build_inputs():
    """{name: case} of every case but the all-kinds one (which the generator
    takes from tests/test_gpu_joint.py's construction)."""
    cases = _geometry() + _running() + _dead() + _edges() + _label_counts() + [_prep()]
    return {c["name"]: c for c in cases}


def public_problem(case):
    """(domain, trials, pool rows, keywords) of a PUBLIC case as the package's
    entry points take it: the geometry space as an hp space, the history as
    real ``Trials`` whose losses give the case's split."""
    from hyperopt_amd import Domain, hp
    from tests import joint_util as U
    space = {"a": hp.loguniform("a", -2, 2), "b": hp.quniform("b", 0, 10, 1),
             "c": hp.pchoice("c", [(p, k) for k, p in enumerate(GEO_PCHOICE)])}
    domain = Domain(lambda x: 0, space)

    def cfg(row):
        return {"a": float(row[0]), "b": float(row[1]), "c": int(row[2])}

    trials = U.make_trials(domain, [cfg(r) for r in case["hist"]], case["losses"])
    kw = dict(prior_weight=case["prior_weight"], gamma=0.25, linear_forgetting=case["lf"],
              bandwidth=case["bandwidth"], cat_smoothing=case["smoothing"])
    return domain, trials, [cfg(r) for r in case["pool"]], kw


# -- the fixture -------------------------------------------------------------------
INPUT_KEYS = ("labels", "probs", "hist", "sig", "pool", "onehot", "losses", "sets")
SCALARS = ("lf", "prior_weight", "bandwidth", "smoothing")


def save(path, cases):
    """Write ``cases`` (inputs and expected values) as one compressed .npz; equal
    arrays (the geometry cases' history and pool) are stored once."""
    blobs, index = {}, {}

    def put(a):
        a = np.ascontiguousarray(a)
        key = (a.dtype.str if a.dtype.names is None else "rec", a.shape, a.tobytes())
        if key not in blobs:
            blobs[key] = ("b%d" % len(blobs), a)
        return blobs[key][0]

    for name, c in cases.items():
        e = {k: c[k] for k in SCALARS}
        e["arrays"] = {k: put(v) for k, v in c.items() if isinstance(v, np.ndarray)}
        e["lists"] = {k: [put(a) for a in v] for k, v in c.items() if isinstance(v, list)}
        index[name] = e
    arrays = {k: a for k, a in blobs.values()}
    arrays["index"] = np.frombuffer(json.dumps(index, sort_keys=True).encode(), np.uint8)
    np.savez_compressed(path, **arrays)


_LOADED = {}


def load():
    """{name: case} of the committed fixture, read once."""
    if not _LOADED:
        with np.load(FIXTURE) as z:
            index = json.loads(bytes(z["index"]).decode())
            for name, e in index.items():
                c = {k: e[k] for k in SCALARS}
                c["name"] = name
                for k, b in e["arrays"].items():
                    c[k] = z[b]
                for k, bs in e["lists"].items():
                    c[k] = [z[b] for b in bs]
                _LOADED[name] = c
    return _LOADED


# -- the same definition in fp64, twice --------------------------------------------
class _Hist(object):
    def __init__(self, vals):
        self.vals = vals


def models_of(case):
    """joint.LabelModel objects equal to the case's label records (column d of
    the values handed to joint._set_log_l is label d)."""
    from hyperopt_amd import joint as J
    out = []
    for d, r in enumerate(case["labels"]):
        m = J.LabelModel()
        m.label, m.col, m.kind = "l%d" % d, int(r["col"]), int(r["kind"])
        m.is_log, m.bounded = bool(r["flags"] & L.JOINT_LOG), bool(r["flags"] & L.JOINT_BOUNDED)
        m.lo, m.hi, m.q = float(r["lo"]), float(r["hi"]), float(r["q"])
        m.mu, m.sigma = float(r["prior_mu"]), float(r["prior_sigma"])
        m.n_cat, m.offset = int(r["n_cat"]), int(r["shift"])
        m.p = label_probs(case, d) if m.kind == L.JOINT_CAT else None
        out.append(m)
    return out


def numpy_log_l(case, s):
    """joint.score_numpy's log L of set s (its ``_set_log_l``, which takes label
    models in place of a Domain)."""
    from hyperopt_amd import joint as J
    models = models_of(case)
    cols = [m.col for m in models]
    x = case["pool"][:, cols] + np.asarray([m.offset for m in models], float)[None, :]
    return J._set_log_l(models, _Hist(case["hist"]), np.asarray(case["sets"][s], np.int64), x,
                        case["lf"], case["prior_weight"], case["bandwidth"], case["smoothing"])


def infos_of(case):
    """tests/joint_util.py's label dicts of the case's records."""
    out = []
    for d, r in enumerate(case["labels"]):
        kind = int(r["kind"])
        info = dict(cls=("cont", "quant", "cat")[kind], log=bool(r["flags"] & L.JOINT_LOG),
                    bounded=bool(r["flags"] & L.JOINT_BOUNDED), lo=float(r["lo"]),
                    hi=float(r["hi"]), q=float(r["q"]) if kind == L.JOINT_QUANT else None,
                    mu=float(r["prior_mu"]), sigma=float(r["prior_sigma"]), K=int(r["n_cat"]),
                    p=None, low=0)
        if kind == L.JOINT_CAT:
            info["p"] = [float(v) for v in label_probs(case, d)]
        out.append(info)
    return out


def scalar_a(case, s, logw=None):
    """(P, C) a_i of set s by tests/joint_util.py's scalar functions (fp64); the
    weights are joint.log_weights' unless ``logw`` is given."""
    from hyperopt_amd import joint as J
    from tests import joint_util as U
    infos, lab = infos_of(case), case["labels"]
    rows = case["sets"][s]
    n = rows.size
    if logw is None:
        logw = J.log_weights(n, case["lf"], case["prior_weight"])
    comps = []
    for d, info in enumerate(infos):
        sigma, col, one = float(case["sig"][s][d]), int(lab["col"][d]), []
        for r in rows:
            obs = float(case["hist"][r, col]) - float(lab["shift"][d])
            if info["cls"] == "cat":
                one.append((False, int(round(obs)), 0.0, 0.0))
            else:
                mu = U.fit(info, obs)
                one.append((False, mu, sigma, U.log_z(info, mu, sigma)))
        one.append((True, info["mu"], info["sigma"],
                    0.0 if info["cls"] == "cat" else U.log_z(info, info["mu"], info["sigma"])))
        comps.append(one)
    a = np.empty((P, n + 1))
    for r in range(P):
        x = [float(case["pool"][r, int(c)]) for c in lab["col"]]
        for i in range(n + 1):
            acc = float(logw[i])
            for d, info in enumerate(infos):
                acc = acc + U.factor(info, x[d], comps[d][i], case["smoothing"])
            a[r, i] = acc
    return a


def scalar_log_l(a):
    """log L per row of the (P, C) matrix ``a``, summed in component order."""
    out = np.empty(a.shape[0])
    for r, row in enumerate(a):
        m = row.max()
        if m == -np.inf:
            out[r] = -np.inf
            continue
        tot = 0.0
        for v in row:
            tot = tot + math.exp(v - m)
        out[r] = m + math.log(tot)
    return out


def k_of(got, ref, cond):
    """The largest |got - ref| / (2**-53 cond) over the finite entries of ``ref``,
    after asserting that -inf and NaN sit where ``ref`` has them."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    fin = np.isfinite(ref)
    assert np.isfinite(got[fin]).all()
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - ref[fin]) / (U53 * np.asarray(cond)[fin])).max())
