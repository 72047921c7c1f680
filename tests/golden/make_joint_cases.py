"""Expected values of tests/joint_cases.py's cases, with mpmath at 50 digits.

    python tests/golden/make_joint_cases.py        writes tests/golden/joint_cases.npz
    python tests/golden/make_joint_cases.py PATH   writes PATH (to compare)

The file is written with fixed zip timestamps: a second run reproduces it bit
for bit.

The definition (include/tpe_hip.h) once more, on mpmath numbers.
Inputs are the fp64 numbers the kernels are handed -- history and pool values,
the label records, the trial components' sigma -- taken exactly; everything
computed from them is computed here at 50 digits and rounded to fp64 once:

  log w_i      log(v_i / (sum v + prior_weight)), v the linear-forgetting ramp
  mu_i         t(obs_i - shift), t = log(max(., 1e-12)) for a log kind
  continuous   -z^2 / 2 - log(sigma sqrt(2 pi)) - log Z
  quantized    log(Phi(ub) - Phi(lb)) - log Z, edges clipped when bounded; an
               unbounded log kind's lower edge <= 0 gives Phi_l = 0
  discrete     log((1[x == c_i] + a p_x) / (1 + a)); the prior: log p_x
  a_i          log w_i + sum_d log k_{d,i};  log L = log sum_i exp(a_i)

A mass of exactly 0.  The model's "a mass <= 0 gives -inf" is a statement
about fp64: in exact arithmetic a normal mass is never 0.  A quantized factor
is -inf here when both clipped edges coincide, or when both edges lie 7 or
more units of sqrt(2) sigma on one side of mu (1 - erf(7) = 4e-23: every fp64
erf returns exactly +-1 there, so every fp64 evaluation gives 0).  Between that
and a mass of 2**-45 an fp64 evaluation may give 0 or rounding noise: Phi is a
multiple of 2**-53 or 2**-54 there and erf is good to an ulp, so the noise is
at most 2**-51.  Such a factor is allowed only in a component that stays below
2**-53 of its row's L even with a mass of 2**-51 in place of the true one: it
then moves log L by less than 2**-53, a small fraction of any tolerance here
(cond >= 1), and the row's fp64 value does not depend on it.  A designed case
with any other such factor is refused here; of the all-kinds case (bandwidth
0.25 in 12 dimensions: most of its rows have one) such rows are not among the
40.

cond(row) = 1 + |log L| + sum_i p_i (|log w_i| + sum_d c_{d,i}), p_i = exp(a_i -
log L); c = 1 + |log k|, plus (Phi_u + Phi_l) / (Phi_u - Phi_l) for a quantized
factor and (Phi_hi + Phi_lo) / Z for a bounded one: first-order propagation of
one rounding per operation.  A one-hot entry (log w_i = 0, the others -inf):
a_i = sum_d log k_{d,i}, cond = 1 + |a_i| + sum_d c_{d,i}.  Prep entries: mu as
above (cond 1 + |mu|); the constant -log(sigma sqrt(2 pi)) - log Z (quantized:
-log Z, discrete: 0) with cond 1 + |log(sigma sqrt(2 pi))| + |log Z| + (Phi_hi +
Phi_lo) / Z.
"""
import io
import os
import sys
import zipfile

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from hyperopt_amd import _lib as L  # noqa: E402
from tests import joint_cases as JC  # noqa: E402

mp.mp.dps = 50
SQRT2 = mp.sqrt(2)
EPS = mp.mpf(1e-12)
LN2 = mp.log(2)
DEAD_Z = 7
NEG_INF = float("-inf")


class BadRow(Exception):
    pass


def F(x):
    return mp.mpf(float(x))


def fit(is_log, v):
    return mp.log(max(v, EPS)) if is_log else v


def phi(z):
    """Phi at (v - mu) / (sqrt(2) sigma) = z."""
    return mp.erfc(-z) / 2


def mass_between(zl, zu):
    if zl is None:
        return phi(zu)
    if zl > 0:
        return (mp.erfc(zl) - mp.erfc(zu)) / 2
    return (mp.erfc(-zu) - mp.erfc(-zl)) / 2


def ramp(n, lf):
    if n < lf:
        return [mp.mpf(1)] * n
    num = n - lf
    first = mp.mpf(1) / n
    step = (1 - first) / (num - 1) if num > 1 else mp.mpf(0)
    return [first + k * step for k in range(num)] + [mp.mpf(1)] * lf


def log_weights(n, lf, prior_weight):
    v = ramp(n, lf) + [F(prior_weight)]
    total = mp.fsum(v)
    return [mp.log(x / total) for x in v]


def components(case, s):
    """Per label the list of (mu, sigma, -log Z, (Phi_hi + Phi_lo) / Z) of set s's
    components, the prior last; a discrete label: (category, ...)."""
    lab, rows = case["labels"], case["sets"][s]
    out = []
    for d, r in enumerate(lab):
        is_log, bounded = bool(r["flags"] & L.JOINT_LOG), bool(r["flags"] & L.JOINT_BOUNDED)
        one = []
        for i in range(len(rows) + 1):
            if i < len(rows):
                obs = F(case["hist"][rows[i], r["col"]]) - F(r["shift"])
                sigma = F(case["sig"][s][d])
            else:
                obs, sigma = None, F(r["prior_sigma"])
            if r["kind"] == L.JOINT_CAT:
                one.append((-1 if obs is None else int(mp.nint(obs)), None, mp.mpf(0), mp.mpf(0)))
                continue
            mu = F(r["prior_mu"]) if obs is None else fit(is_log, obs)
            nlz = zc = mp.mpf(0)
            if bounded:
                zh, zl = (F(r["hi"]) - mu) / (SQRT2 * sigma), (F(r["lo"]) - mu) / (SQRT2 * sigma)
                Z = mass_between(zl, zh)
                nlz, zc = -mp.log(Z), (phi(zh) + phi(zl)) / Z
            one.append((mu, sigma, nlz, zc))
        out.append(one)
    return out


def row_terms(case, d, x):
    """What a factor of label d needs of the row value x."""
    r = case["labels"][d]
    is_log, bounded = bool(r["flags"] & L.JOINT_LOG), bool(r["flags"] & L.JOINT_BOUNDED)
    x = F(x)
    if r["kind"] == L.JOINT_CAT:
        c, a = int(mp.nint(x)), F(case["smoothing"])
        px = F(JC.label_probs(case, d)[c])
        lg = lambda v: mp.log(v) if v > 0 else None  # noqa: E731
        return c, lg((1 + a * px) / (1 + a)), lg(a * px / (1 + a)), lg(px)
    if r["kind"] == L.JOINT_CONT:
        return (fit(is_log, x),)
    q = F(r["q"])
    tu, tl = fit(is_log, x + q / 2), fit(is_log, x - q / 2)
    zero_low = False
    if bounded:
        lo, hi = F(r["lo"]), F(r["hi"])
        tu, tl = min(max(tu, lo), hi), min(max(tl, lo), hi)
    elif is_log and x - q / 2 <= 0:
        zero_low = True
    return tu, tl, zero_low


def factor(kind, rt, comp, is_prior):
    """(log k or None for -inf, c, gray) -- gray: None, or the log of how much
    more an fp64 evaluation of the mass may give."""
    mu, sigma, nlz, zc = comp
    if kind == L.JOINT_CAT:
        c, hit, miss, prior = rt
        lk = prior if is_prior else (hit if c == mu else miss)
        return lk, (1 + abs(lk) if lk is not None else 0), None
    if kind == L.JOINT_CONT:
        z = (rt[0] - mu) / sigma
        lk = -z * z / 2 - mp.log(sigma * mp.sqrt(2 * mp.pi)) + nlz
        return lk, 1 + abs(lk) + zc, None
    tu, tl, zero_low = rt
    zu = (tu - mu) / (SQRT2 * sigma)
    zl = None if zero_low else (tl - mu) / (SQRT2 * sigma)
    if (zl is not None and (tu == tl or zl >= DEAD_Z)) or zu <= -DEAD_Z:
        return None, 0, None
    m = mass_between(zl, zu)
    lk = mp.log(m) + nlz
    ratio = (phi(zu) + (0 if zl is None else phi(zl))) / m
    gray = None
    if m < mp.mpf(2) ** -45:
        gray = max(mp.mpf(0), -51 * LN2 - mp.log(m))
    return lk, 1 + abs(lk) + ratio + zc, gray


def score_set(case, s, rows=None, onehot=()):
    """(log L, cond, one-hot a, one-hot cond) of pool rows ``rows`` under set s;
    a row that depends on a gray factor raises BadRow."""
    lab = case["labels"]
    kinds = [int(k) for k in lab["kind"]]
    comps = components(case, s)
    n = len(case["sets"][s])
    logw = log_weights(n, case["lf"], case["prior_weight"])
    rows = range(case["pool"].shape[0]) if rows is None else rows
    logl, cond = [], []
    oh_a, oh_c = [[] for _ in onehot], [[] for _ in onehot]
    for r in rows:
        rts = [row_terms(case, d, case["pool"][r, lab["col"][d]]) for d in range(len(lab))]
        a, cost, worst = [], [], []
        for i in range(n + 1):
            acc, c, g, dead = logw[i], abs(logw[i]), mp.mpf(0), False
            for d, k in enumerate(kinds):
                lk, cd, gray = factor(k, rts[d], comps[d][i], i == n)
                if lk is None:
                    dead = True
                    break
                acc, c = acc + lk, c + cd
                if gray is not None:
                    g = g + gray
            a.append(None if dead else acc)
            cost.append(c)
            worst.append(g if (not dead and g > 0) else None)
        live = [v for v in a if v is not None]
        if not live:
            logl.append(NEG_INF)
            cond.append(1.0)
        else:
            top = max(live)
            ll = top + mp.log(mp.fsum(mp.exp(v - top) for v in live))
            for v, g in zip(a, worst):
                if g is not None and v + g - ll > -53 * LN2:
                    raise BadRow("%s set %d row %d rests on a mass fp64 cannot form"
                                 % (case["name"], s, r))
            cd = 1 + abs(ll) + mp.fsum(mp.exp(v - ll) * c for v, c in zip(a, cost)
                                       if v is not None)
            logl.append(float(ll))
            cond.append(float(cd))
        for j, i in enumerate(onehot):
            if a[i] is None:
                oh_a[j].append(NEG_INF)
                oh_c[j].append(1.0)
            else:
                if worst[i] is not None:
                    raise BadRow("%s one-hot %d row %d" % (case["name"], i, r))
                v = a[i] - logw[i]
                oh_a[j].append(float(v))
                oh_c[j].append(float(1 + abs(v) + cost[i] - abs(logw[i])))
    return np.asarray(logl), np.asarray(cond), np.asarray(oh_a), np.asarray(oh_c)


def prep_expected(case, s):
    """(mu, constant, cond of the constant), each (D, C), of set s."""
    lab = case["labels"]
    comps = components(case, s)
    C = len(case["sets"][s]) + 1
    mu, cst, cc = (np.zeros((len(lab), C)) for _ in range(3))
    for d, r in enumerate(lab):
        for i, (m, sigma, nlz, zc) in enumerate(comps[d]):
            mu[d, i] = float(m)
            if r["kind"] == L.JOINT_CAT:
                continue
            ls = mp.log(sigma * mp.sqrt(2 * mp.pi)) if r["kind"] == L.JOINT_CONT else mp.mpf(0)
            cst[d, i] = float(nlz - ls)
            cc[d, i] = float(1 + abs(ls) + abs(nlz) + zc)
    return mu, cst, cc.astype(np.float32)


def expected(case):
    """Add the expected values to ``case``."""
    case["logl"], case["cond"] = [], []
    for s in range(len(case["sets"])):
        oh = [int(i) for i in case["onehot"]] if s == 0 else ()
        ll, cd, oa, oc = score_set(case, s, onehot=oh)
        case["logl"].append(ll)
        case["cond"].append(cd)
        if oh:
            case["onehot_a"], case["onehot_cond"] = oa, oc
    if case["name"] == "prep":
        case["prep_mu"], case["prep_cst"], case["prep_cond"] = [], [], []
        for s in range(len(case["sets"])):
            for k, v in zip(("prep_mu", "prep_cst", "prep_cond"), prep_expected(case, s)):
                case[k].append(v)
    return case


# -- the all-kinds case of tests/test_gpu_joint.py ----------------------------------
def all_kinds_case():
    """tests/test_gpu_joint.py's all-kinds case as a case of the table (the
    package builds its history, split and label records), and 40 of its 300 rows:
    5, 150 and 299, which that file names, then the first rows that do not rest
    on a gray factor and have cond <= 1e6."""
    from hyperopt_amd import Domain, hp, rand, tpe
    from hyperopt_amd import joint as J
    from tests import joint_util as U
    kw = dict(prior_weight=0.7, gamma=0.25, linear_forgetting=25, bandwidth=0.25, cat_smoothing=0.5)
    domain = Domain(lambda x: 0, U.all_kinds_space(hp))
    rng = np.random.RandomState(17)
    configs = [rand.sample_config(domain, rng) for _ in range(620)]
    losses = rng.uniform(size=620)
    losses[[40, 333]] = np.inf
    trials = U.make_trials(domain, configs, losses)
    rows = [rand.sample_config(domain, rng) for _ in range(300)]
    rows[5]["i"], rows[299]["k"], rows[150]["g"] = 2.0e6, 0, -60.0
    pool = tpe.Pool(domain, rows)
    hist = tpe.collect_history(trials, pool.labels)
    models = J.label_models(domain)
    specs = []
    for m in models:
        specs.append(JC._spec(m.kind, log=m.is_log, bounded=m.bounded, lo=m.lo, hi=m.hi, q=m.q,
                              mu=m.mu, sigma=m.sigma, p=m.p, shift=m.offset))
    cols = [m.col for m in models]
    isb, isa = tpe.split_masks(hist, kw["gamma"])
    sets = [J.set_rows(hist, mask, cols) for mask in (isb, isa)]
    dev = np.asarray(pool.vals, np.float64).copy()
    for m in models:
        dev[:, m.col] -= m.offset
    case = dict(name="all_kinds", hist=np.asarray(hist.vals, np.float64),
                sets=[np.asarray(s, np.int32) for s in sets], lf=25, prior_weight=0.7,
                bandwidth=0.25, smoothing=0.5, onehot=np.zeros(0, np.int64))
    case["labels"], case["probs"] = JC.records(specs, cols)
    case["sig"] = np.stack([JC.bandwidths(case["labels"], s.size, 0.25) for s in case["sets"]])
    case["pool"] = dev
    picked, out = [], {}
    for r in [5, 150, 299] + [r for r in range(300) if r not in (5, 150, 299)]:
        try:
            got = [score_set(case, s, rows=[r])[:2] for s in (0, 1)]
        except BadRow:
            continue
        if max(float(g[1][0]) for g in got) > 1e6:
            continue
        picked.append(r)
        out[r] = got
        if len(picked) == JC.P:
            break
    assert len(picked) == JC.P, len(picked)
    picked.sort()
    case["row_ids"] = np.asarray(picked, np.int64)
    case["pool"] = dev[picked]
    case["logl"] = [np.asarray([out[r][s][0][0] for r in picked]) for s in (0, 1)]
    case["cond"] = [np.asarray([out[r][s][1][0] for r in picked]) for s in (0, 1)]
    return case


def write(path, cases):
    """JC.save with fixed zip timestamps."""
    buf = io.BytesIO()
    JC.save(buf, cases)
    buf.seek(0)
    with np.load(buf) as z, zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as out:
        for key in sorted(z.files):
            raw = io.BytesIO()
            np.lib.format.write_array(raw, z[key], allow_pickle=False)
            out.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)),
                         raw.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def main(path):
    cases = JC.build_inputs()
    for name, case in cases.items():
        expected(case)
        print(name, "max cond %.3g" % max(float(c.max()) for c in case["cond"]), flush=True)
    cases["all_kinds"] = all_kinds_case()
    write(path, cases)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else JC.FIXTURE)
