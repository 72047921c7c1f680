"""Characterisation records of the four search algorithms' host side: what
tpe.suggest / tpe.suggest_many hand to Engine.run, what rand and anneal ask of
their device calls, and the trial documents every entry point returns --
captured without a GPU.

``tpe.engine`` returns one stand-in engine of tools/host_cpu_profile.py per
slot whose ``run`` is a recorder; ``rand.draw_priors``, ``anneal.sample_level``,
``dist.world``, ``dist.gather_best`` and ``dist.allreduce_best`` are patched
too.  The recorder logs the WorkBatch (key with level ids renumbered by first
appearance, counts, Philox keys, candidate bases, every field of every
materialised LabelWork) or the work list, and the run keyword arguments
(histories as indices, row lists and split flags as hashes).  It answers with
a winner per label that is a fixed function of the label's Philox key --
``key % K`` for randint / categorical, a value inside the prior's support
otherwise -- so nested spaces walk down different branches.

    python tests/golden/make_suggest_records.py      # rewrite suggest_records.json

It uses only names that the refactor of the algorithm modules keeps (the
entry points and the patched names above), so the same file runs before and
after; tests/golden/suggest_records.json was written by the commit before
hyperopt_amd/walk.py existed and is never regenerated from later code
(tests/test_suggest_records.py compares against it).
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import host_cpu_profile as H  # noqa: E402
from hyperopt_amd import _lib as L  # noqa: E402
from hyperopt_amd import anneal, hp, mix, rand, tpe  # noqa: E402
from hyperopt_amd import dist as hdist  # noqa: E402
from hyperopt_amd import engine as E  # noqa: E402
from hyperopt_amd.base import JOB_STATE_DONE, JOB_STATE_NEW, Domain, Trials  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "suggest_records.json")


def _sha(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return [str(a.dtype), list(a.shape), hashlib.sha256(a.tobytes()).hexdigest()[:12]]


def _plain(v):
    if isinstance(v, np.ndarray):
        return [_plain(x) for x in v.tolist()]
    if isinstance(v, (np.floating, np.integer, np.bool_)):
        return _plain(v.item())
    if isinstance(v, float) and v != v:
        return "nan"
    if isinstance(v, float) and v in (float("inf"), float("-inf")):
        return "inf" if v > 0 else "-inf"
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}  # (insertion order kept)
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def winner(kind, args, key):
    """The stand-in's winning engine value of a label: a fixed function of
    its Philox key, inside the prior's support."""
    key = int(key)
    if kind == "randint":
        n = int(args[0]) if (len(args) < 2 or args[1] is None) else int(args[1]) - int(args[0])
        return float(key % n)
    if kind == "categorical":
        p = np.asarray(args[0], dtype=np.float64)
        return float(key % (p.shape[-1] if p.ndim == 2 else p.size))
    f = ((key >> 7) % 1000 + 0.5) / 1000.0
    if kind in ("uniform", "quniform", "loguniform", "qloguniform"):
        v = args[0] + f * (args[1] - args[0])
    else:
        v = args[0] + args[1] * (2.0 * f - 1.0)
    if "log" in kind:
        v = float(np.exp(v))
    if kind.startswith("q"):
        v = float(np.round(v / args[2]) * args[2])
    return float(v)


class Recorder(object):
    """The patched names of one case and the log they write."""

    def __init__(self, world=(0, 1)):
        self.log = []
        self.hists = []      # device histories by first appearance (kept alive)
        self.level_ids = {}  # engine level id -> first-appearance number
        self.world = world
        self.engines = {}

    # -- tpe.engine ----------------------------------------------------------------
    def engine(self, slot=0):
        eng = self.engines.get(slot)
        if eng is None:
            eng = self.engines[slot] = H.make_engine()
            eng.run = lambda works, **kw: self.run(slot, works, **kw)
        return eng

    def _hist(self, h):
        if h is None:
            return None
        for i, x in enumerate(self.hists):
            if x is h:
                return i
        self.hists.append(h)
        return len(self.hists) - 1

    def _lid(self, lid):
        return self.level_ids.setdefault(lid, len(self.level_ids))

    def _key(self, key):
        if key and key[0] == "suggest":  # ("suggest", level id, units, n_ei, lat)
            return ["suggest", self._lid(key[1])] + _plain(list(key[2:]))
        return [[self._lid(k[0])] + _plain(list(k[1:])) for k in key]

    @staticmethod
    def _work(w):
        return {"label": w.label, "kind": w.kind, "args": _plain(w.args),
                "obs_below": _sha(w.obs_below), "obs_above": _sha(w.obs_above),
                "n_cand": int(w.n_cand), "key": int(w.key), "cand_base": int(w.cand_base),
                "cand": _sha(w.cand), "col": _plain(w.col), "n_above": int(w.n_above),
                "hist": int(w.hist), "n_total": int(w.n_total)}

    def run(self, slot, works, **kw):
        row = {"slot": slot}
        batch = isinstance(works, E.WorkBatch)
        if batch:
            row["batch"] = {"key": self._key(works.key), "n_below": _plain(works.n_below),
                            "n_above": _plain(works.n_above), "keys": _plain(works.keys),
                            "cand_base": _plain(works.cand_base)}
            ws = works.materialize()
            assert len(ws) == len(works)
        else:
            ws = works
        row["works"] = [self._work(w) for w in ws]
        k = {}
        for name, v in kw.items():  # (in the order they were given)
            if name == "history":
                k[name] = self._hist(v)
            elif name in ("rows", "is_below"):
                k[name] = _sha(v)
            elif name == "histories":
                k[name] = [[self._hist(h), _sha(r), _sha(f)] for h, r, f in v]
            else:
                k[name] = _plain(v)
        row["kwargs"] = k
        self.log.append(row)
        vals = [winner(w.kind, w.args, w.key) for w in ws]
        if not batch:
            return [E.LabelResult(w.label, int(w.key % max(w.n_cand, 1)) + int(w.cand_base), v,
                                  float((w.key >> 11) % 997), int(w.n_cand))
                    for w, v in zip(ws, vals)]
        res = E.BatchResult(np.array([int(w.key % max(w.n_cand, 1)) for w in ws], np.int64),
                            np.array(vals, np.float64),
                            np.array([float((w.key >> 11) % 997) for w in ws]),
                            np.array([w.n_cand for w in ws], np.int64))
        return _Deferred(res) if kw.get("defer") else res

    # -- rand / anneal / dist ------------------------------------------------------------
    def draw_priors(self, domain, seed, n):
        labels = list(domain.params)
        keys = tpe.label_keys(seed, labels)
        self.log.append({"draw_priors": labels, "seed": int(seed), "n": int(n)})
        out = np.zeros((len(labels), n))
        for j, lab in enumerate(labels):
            spec = domain.specs[lab]
            for i in range(n):
                v = winner(spec.kind, spec.args, keys[j] + 7919 * (i + 1))
                if spec.kind == "randint" and len(spec.args) > 1 and spec.args[1] is not None:
                    v += int(spec.args[0])  # (the prior kernel draws in [low, high))
                out[j, i] = v
        return labels, out

    def sample_level_for(self, domain):
        labels = list(domain.params)

        def sample_level(eng, dh, loss, rec, pool, items, new_ids, avg_best_idx, state,
                         debug=False):
            assert not debug
            self.log.append({"sample_level": _plain(items), "new_ids": _plain(list(new_ids)),
                             "history": self._hist(dh), "rows": int(dh.rows),
                             "loss": _sha(loss.numpy()[:dh.rows]), "pool": _sha(pool),
                             "rec": {n: _plain(rec[n]) for n in rec.dtype.names},
                             "avg_best_idx": float(avg_best_idx)})
            out = []
            for it, new_id in zip(items, new_ids):
                for j in it:
                    spec = domain.specs[labels[j]]
                    v = winner(spec.kind, spec.args, int(rec["key"][j]) + 104729 * (new_id + 1))
                    if spec.kind == "randint" and spec.args[1] is not None:
                        v += int(spec.args[0])
                    out.append(v)
            return np.array(out, np.float64)
        return sample_level

    def gather_best(self, n_labels, local, group=None):
        """dist.gather_best without the all-gather: this rank's records."""
        rec = hdist.empty_records(n_labels)
        for i, r in local:
            cur = rec[i]
            if hdist.better(r.score, r.index, cur["score"], cur["index"]):
                rec[i] = (r.score, r.index, r.value, cur["n_scored"] + r.n_scored)
            else:
                rec[i]["n_scored"] = cur["n_scored"] + r.n_scored
        out = [(float(x["score"]), int(x["index"]), float(x["value"]), int(x["n_scored"]))
               for x in rec]
        self.log.append({"gather_best": n_labels, "local": [i for i, _ in local],
                         "best": _plain(out)})
        return out

    def allreduce_best(self, results, group=None):
        self.log.append({"allreduce_best": [r.label for r in results]})
        return results


class _Deferred(object):
    def __init__(self, res):
        self._res = res

    def result(self):
        return self._res


# -- spaces and histories ----------------------------------------------------------
def flat_space():
    return {"x": hp.uniform("x", -5, 5), "lr": hp.loguniform("lr", -7, 0),
            "k": hp.randint("k", 6), "q": hp.quniform("q", 0, 20, 2)}


def nested_space():
    """Three levels: a -> (b | c) -> (d | e), plus a label that is always live."""
    return {"top": hp.uniform("top", 0, 1),
            "a": hp.choice("a", [
                {"b": hp.choice("b", [{"d": hp.normal("d", 0, 1)},
                                      {"e": hp.randint("e", 3, 9)}])},
                {"c": hp.quniform("c", 1, 9, 1), "f": hp.lognormal("f", 0, 1)}])}


def kinds_space():
    return {"u": hp.uniform("u", -5, 5), "qlu": hp.qloguniform("qlu", 0, 4, 1),
            "n": hp.normal("n", 0, 2), "qn": hp.qnormal("qn", 0, 5, 1),
            "qln": hp.qlognormal("qln", 0, 1, 1), "r": hp.randint("r", 3, 11),
            "pc": hp.pchoice("pc", [(0.2, "a"), (0.3, "b"), (0.5, "c")]),
            "ln": hp.lognormal("ln", 0, 1)}


def lattice_space():
    # hashable prior arguments and unbounded quantized labels: the WorkBatch's lat tuple
    return {"qn": hp.qnormal("qn", 0, 5, 1), "u": hp.uniform("u", -5, 5),
            "qln": hp.qlognormal("qln", 0, 1, 1), "r": hp.randint("r", 3, 11),
            "c": hp.choice("c", [{"qn2": hp.qnormal("qn2", 2, 3, 0.5)}, {"z": hp.randint("z", 4)}])}


def small_space():
    return {"x": hp.uniform("x", 0, 1), "c": hp.choice("c", [{"y": hp.normal("y", 0, 1)}, 1])}


def unhashable_space():
    # a list as a prior argument: _space_sig is None, so the work-list path
    return {"x": hp.uniform("x", -1, 1), "pc": hp.pchoice("pc", [(0.5, 0), (0.5, 1)]),
            "q": hp.quniform("q", 0, 10, 1)}


class ForeignTrials(object):
    """A Trials class from another package: documents, no columnar()."""

    def __init__(self):
        self._docs = []

    @property
    def trials(self):
        return self._docs

    def __len__(self):
        return len(self._docs)

    def new_trial_docs(self, tids, specs, results, miscs):
        return [{"state": JOB_STATE_NEW, "tid": t, "spec": s, "result": r, "misc": m,
                 "exp_key": None, "owner": None, "version": 0, "book_time": None,
                 "refresh_time": None, "foreign": True}
                for t, s, r, m in zip(tids, specs, results, miscs)]

    def insert_trial_docs(self, docs):
        self._docs.extend(docs)

    def refresh(self):
        pass


class _slot_trials(object):
    """... that can be neither weak-referenced nor given an attribute: no
    columnar cache at all, host observation lists."""
    __slots__ = ("_docs",)
    __init__ = ForeignTrials.__init__
    trials = ForeignTrials.trials
    __len__ = ForeignTrials.__len__
    new_trial_docs = ForeignTrials.new_trial_docs
    insert_trial_docs = ForeignTrials.insert_trial_docs
    refresh = ForeignTrials.refresh


def make_history(space, T, seed, trials=None, losses=None, alias=()):
    """(domain, trials) with T finished documents drawn from the priors;
    ``losses``: {tid: loss} overrides (None, NaN); ``alias``: (tid, from_tid)
    documents appended after them."""
    domain = Domain(lambda p: 0.0, space)
    trials = Trials() if trials is None else trials
    rng = np.random.RandomState(seed)
    labels = list(domain.params)
    docs = []

    def doc(tid, config, loss, from_tid=None):
        misc = {"tid": tid, "cmd": domain.cmd, "workdir": None,
                "idxs": {lab: ([tid] if lab in config else []) for lab in labels},
                "vals": {lab: ([config[lab]] if lab in config else []) for lab in labels}}
        if from_tid is not None:
            misc["from_tid"] = from_tid
        d = trials.new_trial_docs([tid], [None], [{"status": "ok", "loss": loss}], [misc])[0]
        d["state"] = JOB_STATE_DONE
        return d
    for tid in range(T):
        config = rand.sample_config(domain, rng)
        loss = float(rng.normal())
        if losses and tid in losses:
            loss = losses[tid]
        docs.append(doc(tid, config, loss))
    for k, (tid, src) in enumerate(alias):
        docs.append(doc(tid, rand.sample_config(domain, rng), float(rng.normal()) - 1.0, src))
    trials.insert_trial_docs(docs)
    trials.refresh()
    return domain, trials


# -- the cases ------------------------------------------------------------------------
def _suggest(rec, space, T=40, seed=11, new_ids=None, hist_seed=3, **kw):
    make = kw.pop("make", {})
    domain, trials = make_history(space, T, hist_seed, **make)
    new_ids = [T + 5] if new_ids is None else new_ids
    return tpe.suggest(new_ids, domain, trials, seed, verbose=False, **kw)


def case_flat(rec):
    return _suggest(rec, flat_space())


def case_nested(rec):
    # (several seeds: different branches)
    return [_suggest(rec, nested_space(), T=60, seed=s) for s in (1, 2, 3, 4)]


def case_kinds(rec):
    return _suggest(rec, kinds_space(), T=50, gamma=0.5, prior_weight=0.7,
                    linear_forgetting=20)


def case_lattice(rec):
    return [_suggest(rec, lattice_space(), T=50, seed=s) for s in (1, 2)]


def case_kinds_big(rec):
    return _suggest(rec, kinds_space(), T=50, n_EI_candidates=1 << 17, precision=32)


def case_alias_nan(rec):
    return _suggest(rec, nested_space(), T=45, make=dict(
        losses={3: None, 7: float("nan"), 0: float("nan"), 12: None},
        alias=((45, 4), (46, 9), (47, 9))))


def case_nan_only(rec):
    # (NaN losses without from_tid rows: a row list over the cache)
    return _suggest(rec, flat_space(), T=30, make=dict(losses={5: float("nan"), 6: None}))


def case_unhashable(rec):
    return _suggest(rec, unhashable_space(), T=30)


def case_foreign(rec):
    return _suggest(rec, nested_space(), T=40, make=dict(trials=ForeignTrials()))


def case_foreign_no_cache(rec):
    return _suggest(rec, nested_space(), T=40, make=dict(trials=_slot_trials()))


def case_zero_candidates(rec):
    return _suggest(rec, nested_space(), n_EI_candidates=0)


def case_startup(rec):
    return _suggest(rec, nested_space(), T=12, new_ids=[12, 13, 14])


def case_world_1_of_2(rec):
    return [_suggest(rec, sp, T=40, seed=s) for sp, s in
            ((nested_space(), 2), (kinds_space(), 5), (small_space(), 6))]


case_world_2_of_3 = case_world_1_of_2


def _requests():
    d0, t0 = make_history(nested_space(), 60, 21)
    d1, t1 = make_history(flat_space(), 30, 22)
    d2, t2 = make_history(kinds_space(), 45, 23)
    d3, t3 = make_history(small_space(), 8, 24)   # startup phase
    d4, t4 = make_history(unhashable_space(), 25, 25)
    d5, t5 = make_history(nested_space(), 33, 26, trials=ForeignTrials())
    d7, t7 = make_history(lattice_space(), 44, 27)
    return [tpe.SuggestRequest([60], d0, t0, 100),
            tpe.SuggestRequest([30], d1, t1, 101, gamma=0.5, n_EI_candidates=50),
            tpe.SuggestRequest([45], d2, t2, 102, prior_weight=0.5, linear_forgetting=10,
                               verbose=True),
            tpe.SuggestRequest([8, 9], d3, t3, 103),
            tpe.SuggestRequest([25], d4, t4, 104),
            tpe.SuggestRequest([33], d5, t5, 105, n_EI_candidates=0),
            tpe.SuggestRequest([60], d0, t0, 106, precision=32),
            tpe.SuggestRequest([44], d7, t7, 107, gamma=0.4, n_EI_candidates=30)]


def case_many(rec):
    return tpe.suggest_many(_requests())


def case_many_three(rec):
    return tpe.suggest_many([_requests()[i] for i in (0, 7, 3)])


def case_many_one(rec):
    return tpe.suggest_many(_requests()[:1])


def case_many_chunk2(rec):
    os.environ["HYPEROPT_AMD_CHUNK"] = "2"
    try:
        return tpe.suggest_many(_requests())
    finally:
        del os.environ["HYPEROPT_AMD_CHUNK"]


def case_many_shard_studies(rec):
    return tpe.suggest_many(_requests(), shard_studies=True)


def case_many_world2(rec):
    return tpe.suggest_many(_requests())


def _nested_history(**kw):
    return make_history(nested_space(), 40, 31, **kw)


def case_anneal(rec):
    domain, trials = _nested_history()
    anneal.sample_level = rec.sample_level_for(domain)
    return {"suggest": anneal.suggest([40, 41, 42], domain, trials, 7),
            "suggest_opts": anneal.suggest([43], domain, trials, 8, avg_best_idx=3.0,
                                           shrink_coef=0.2),
            "suggest_batch": anneal.suggest_batch([40, 41, 42], domain, trials, 7)}


def case_anneal_host(rec):
    domain, trials = _nested_history()
    alias = _nested_history(alias=((40, 3), (41, 3)))
    foreign = _nested_history(trials=_slot_trials())
    empty = make_history(nested_space(), 0, 1)
    return {"suggest_host": anneal.suggest_host([40, 41, 42], domain, trials, 7),
            "suggest_alias": anneal.suggest([42, 43, 44], alias[0], alias[1], 7),
            "suggest_batch_alias": anneal.suggest_batch([42, 43, 44], alias[0], alias[1], 9),
            "suggest_no_cache": anneal.suggest([40, 41, 42], foreign[0], foreign[1], 7),
            "suggest_empty": anneal.suggest_host([0, 1, 2], empty[0], empty[1], 5),
            "host_kinds": anneal.suggest_host([50, 51], *make_history(kinds_space(), 50, 3),
                                              seed=4)}


def case_rand(rec):
    domain, trials = _nested_history()
    kd, kt = make_history(kinds_space(), 5, 3)
    return {"suggest": rand.suggest([40, 41, 42], domain, trials, 7),
            "suggest_batch": rand.suggest_batch([40, 41, 42], domain, trials, 7),
            "suggest_device": rand.suggest_device([40, 41, 42], domain, trials, 7),
            "suggest_kinds": rand.suggest([5, 6], kd, kt, 2),
            "suggest_device_kinds": rand.suggest_device([5, 6, 7], kd, kt, 2)}


def case_mix(rec):
    domain, trials = _nested_history()
    anneal.sample_level = rec.sample_level_for(domain)
    p = [(0.3, rand.suggest), (0.3, anneal.suggest), (0.4, tpe.suggest)]
    return [mix.suggest([40 + s], domain, trials, s, p_suggest=p) for s in range(6)]


CASES = {
    "suggest_flat": (case_flat, (0, 1)),
    "suggest_nested": (case_nested, (0, 1)),
    "suggest_kinds": (case_kinds, (0, 1)),
    "suggest_kinds_fp32": (case_kinds_big, (0, 1)),
    "suggest_lattice": (case_lattice, (0, 1)),
    "suggest_alias_nan": (case_alias_nan, (0, 1)),
    "suggest_nan_rows": (case_nan_only, (0, 1)),
    "suggest_unhashable": (case_unhashable, (0, 1)),
    "suggest_foreign": (case_foreign, (0, 1)),
    "suggest_foreign_no_cache": (case_foreign_no_cache, (0, 1)),
    "suggest_zero_candidates": (case_zero_candidates, (0, 1)),
    "suggest_startup": (case_startup, (0, 1)),
    "suggest_world_1_of_2": (case_world_1_of_2, (1, 2)),
    "suggest_world_2_of_3": (case_world_2_of_3, (2, 3)),
    "many": (case_many, (0, 1)),
    "many_three": (case_many_three, (0, 1)),
    "many_one": (case_many_one, (0, 1)),
    "many_chunk2": (case_many_chunk2, (0, 1)),
    "many_shard_studies_0_of_2": (case_many_shard_studies, (0, 2)),
    "many_shard_studies_1_of_2": (case_many_shard_studies, (1, 2)),
    "many_world2": (case_many_world2, (1, 2)),
    "anneal": (case_anneal, (0, 1)),
    "anneal_host": (case_anneal_host, (0, 1)),
    "rand": (case_rand, (0, 1)),
    "mix": (case_mix, (0, 1)),
}

_PATCHED = ((tpe, "engine"), (rand, "draw_priors"), (anneal, "sample_level"), (hdist, "world"),
            (hdist, "gather_best"), (hdist, "allreduce_best"), (L, "hip"))


def capture(name):
    """{"calls": the log, "docs": what the entry points returned} of one case,
    as plain JSON values."""
    fn, world = CASES[name]
    rec = Recorder(world)
    saved = [(m, n, getattr(m, n)) for m, n in _PATCHED]
    tpe.engine = rec.engine
    rand.draw_priors = rec.draw_priors
    hdist.world = lambda: rec.world
    hdist.gather_best = rec.gather_best
    hdist.allreduce_best = rec.allreduce_best
    try:
        docs = fn(rec)
        return json.loads(json.dumps({"calls": _plain(rec.log), "docs": _plain(docs)}))
    finally:
        for m, n, v in saved:
            setattr(m, n, v)


def dump(data):
    """One logged call and one document per line."""
    lines = ["{"]
    for ci, (name, case) in enumerate(data.items()):
        lines.append(" %s: {" % json.dumps(name))
        lines.append('  "calls": [')
        for i, row in enumerate(case["calls"]):
            lines.append("   " + json.dumps(row) + ("," if i + 1 < len(case["calls"]) else ""))
        lines.append("  ],")
        lines.append('  "docs": ' + json.dumps(case["docs"]))
        lines.append(" }" + ("," if ci + 1 < len(data) else ""))
    lines.append("}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    text = dump({name: capture(name) for name in CASES})
    assert json.loads(text) is not None
    with open(path, "w") as f:
        f.write(text)
    print("%s: %d cases, %d bytes" % (path, len(CASES), len(text)))
