"""Characterisation records of the engine's host side: what one Engine.run
call hands to the library and the HIP runtime, captured without a GPU.

The engine runs against the stand-ins of tools/host_cpu_profile.py (CPU
tensors for the workspace) with a library and a runtime that record every
launch entry point and every runtime call, in order, with all arguments.
Addresses are made position-independent: one inside a workspace buffer, a
pinned buffer, a history tensor or a host descriptor table becomes
[name, offset]; events become their name; anything else is "host".  Per call
the records also hold a SHA-256 of the staged pack, ``graph_stats`` and the
returned results (which the stand-ins leave at zero).

    python tests/golden/make_level_records.py          # rewrite level_records.json

It uses only Engine.run, DeviceHistory and make_engine, so the same file
runs on any commit; tests/golden/level_records.json was written by the commit
before the engine's level records were introduced and is never regenerated
from later code (tests/test_level_records.py compares against it).

Not captured (covered by their GPU tests only):
  - TPE_GRAPHS=1: the hipGraph replay needs a real capture (tests/test_gpu_replay.py).
  - band overflow / owed second exchange: the stand-ins leave n_scored at zero,
    so _band_fix and _exchange_fix never fire (tests/test_gpu_table.py, test_gpu_rccl.py).
"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
import host_cpu_profile as H  # noqa: E402
from hyperopt_amd import _lib as L  # noqa: E402
from hyperopt_amd import dist as hdist  # noqa: E402
from hyperopt_amd import engine as E  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "level_records.json")
SIDE = 7            # the side stream's handle in the stand-in runtime
EV_BASE = 1 << 44   # event handles of the stand-in runtime (told apart from sizes)
INT_MAX = 1 << 22   # launch arguments below this are counts and sizes, never addresses
ADDR_MIN = 1 << 40  # anything at least this large is an address (known or not)
COMM = 12345        # the dummy communicator of the exchange level
_CALLS = ("tpe_history_append", "tpe_run_ops", "tpe_ops_capture", "tpe_graph_launch",
          "tpe_graph_destroy")
_OP_NAMES = {code: name for name, code in L.OP_CODES.items()}
_OP_NAMES.update({L.OP_EVENT_RECORD: "op_event_record", L.OP_STREAM_WAIT: "op_stream_wait",
                  L.OP_MEMCPY: "op_memcpy", L.OP_STREAM_SYNC: "op_stream_sync"})


class _SideStream(object):
    cuda_stream = SIDE

    def __init__(self, *a, **k):
        pass


def _sha(data):
    return hashlib.sha256(data).hexdigest()[:16]


class Capture(object):
    """One engine with a recording library and runtime."""

    def __init__(self, hashed=False, **knobs):
        self.eng = eng = H.make_engine()
        eng.torch.cuda.Stream = _SideStream
        for k, v in knobs.items():
            assert hasattr(eng, k), k
            setattr(eng, k, v)
        self.hashed = hashed  # C3-sized levels: one hash per launch instead of its arguments
        self.real = L.load()
        self.log = []
        self.n_events = 0
        self.hists = []
        self.pack_hash = True
        eng.lib = _RecLib(self)
        eng._hip = _RecHip(self)  # (L.hip() of make_engine returns eng._hip)
        upload = eng._upload

        def hooked(pack, stream, slot=0, copy=True):
            dev = upload(pack, stream, slot, copy)
            if self.pack_hash:
                host = eng._pinned[slot].numpy()
                self.log.append(["pack", slot, pack.size, _sha(host[:pack.size].tobytes())])
            return dev
        eng._upload = hooked

    def history(self, n_labels, cap):
        h = E.DeviceHistory(self.eng, n_labels, cap=cap)
        self.hists.append(h)
        return h

    # -- addresses -------------------------------------------------------------
    def _ranges(self):
        eng = self.eng
        out = []

        def tensor(name, t):
            if t is not None:
                out.append((name, t.data_ptr(), t.numel() * t.element_size()))

        def array(name, a):
            if a is not None and getattr(a, "nbytes", 0):
                out.append((name, a.__array_interface__["data"][0], a.nbytes))
        for name, t in eng._bufs.items():
            tensor(name, t)
        for slot, t in eng._pinned.items():
            tensor("pinned%d" % slot, t)
        tensor("res_pin", eng._res_pin)
        for k, h in enumerate(self.hists):
            for name in ("vals", "active", "order", "_stage", "_dstage"):
                tensor("hist%d.%s" % (k, name.strip("_")), getattr(h, name, None))
            # (the column specs of the sorted orders, on the host and the device)
            for i, (arr, dev) in enumerate(h.__dict__.get("_spec_dev", {}).values()):
                array("hist%d.spec%d" % (k, i), arr)
                tensor("hist%d.dspec%d" % (k, i), dev)
        plan = getattr(eng, "last_plan", None)
        if plan is not None:
            for name, a in zip(("segs", "csegs", "g", "jobs"), plan):
                array("plan." + name, a)
        recs = list(eng._oplists.values())
        if eng._oplist_once is not None:
            recs.append(eng._oplist_once)
        for r in recs:
            for name, a in zip(("jobs", "fb", "g", "h"), r.keep or ()):
                array("keep." + name, a)
        return out

    def norm(self, a, ranges):
        if a is None or isinstance(a, (bool, str)):
            return a
        typed = isinstance(a, ctypes.c_void_p)  # a pointer or handle for certain
        if typed:
            a = a.value or 0
        elif isinstance(a, ctypes._SimpleCData):
            a = a.value
        if isinstance(a, (float, np.floating)):
            return float(a)
        if isinstance(a, (int, np.integer)):
            a = int(a)
            if abs(a) < INT_MAX:
                return a
            if EV_BASE <= a < EV_BASE + self.n_events:
                for name, h in self.eng._events.items():
                    if (h.value or 0) == a:
                        return "event:" + name
                return "event#%d" % (a - EV_BASE)
            for name, lo, n in ranges:
                if lo <= a < lo + n:
                    return [name, a - lo]
            for name, lo, n in ranges:  # (the cell pointer of a second table group is biased)
                if name == "cells" and lo - (1 << 30) <= a < lo:
                    return [name, a - lo]
            return "host" if typed or a >= ADDR_MIN else a
        if hasattr(a, "_obj"):  # ctypes.byref(...)
            return "ref"
        return type(a).__name__

    def record(self, name, args):
        ranges = self._ranges()
        row = [name] + [self.norm(a, ranges) for a in args]
        if name == "tpe_run_ops":
            self._add([name, args[1]])
            ops = np.frombuffer((ctypes.c_char * (args[1] * L.OP_DTYPE.itemsize)).from_address(
                args[0]), L.OP_DTYPE)
            for op in ops:
                words = op["a"][:int(op["n_args"])].tolist()
                self._add([_OP_NAMES.get(int(op["code"]), int(op["code"]))] +
                          [self.norm(w, ranges) for w in words], "  ")
            first = ops[0]
            if int(first["code"]) == L.OP_MEMCPY and self.pack_hash:
                src, nb = int(first["a"][1]), int(first["a"][2])
                for pname, lo, n in ranges:
                    if pname == "pinned0" and lo <= src and src + nb <= lo + n:
                        host = self.eng._pinned[0].numpy()
                        self.log.append(["pack", 0, nb,
                                         _sha(host[src - lo:src - lo + nb].tobytes())])
            return
        self._add(row)

    def _add(self, row, indent=""):
        if self.hashed and len(row) > 2:  # [name, stream, hash of the rest]
            last = row[-1] if isinstance(row[-1], int) and not isinstance(row[-1], bool) else None
            row = [row[0], last, _sha(json.dumps(row[1:]).encode())]
        row[0] = indent + row[0]
        self.log.append(row)

    # -- one Engine.run call ------------------------------------------------------
    def run(self, works, collect=True, **kw):
        del self.log[:]
        res = self.eng.run(works, **kw)
        if hasattr(res, "result"):  # a deferred WorkBatch level
            self.log.append(["deferred"])
            res = res.result() if collect else None
        return {"launches": [list(r) for r in self.log], "results": _results(res),
                "graph_stats": dict(self.eng.graph_stats),
                "last": {k: _plain(getattr(self.eng, k, None))
                         for k in ("last_pairs", "last_table_stats", "last_exchange")}}


class _RecLib(object):
    def __init__(self, cap):
        self._cap = cap

    def __getattr__(self, name):
        if name in L.OP_CODES or name in _CALLS:
            def call(*args):
                self._cap.record(name, args)
                return 0
            return call
        return getattr(self._cap.real, name)


class _RecHip(object):
    def __init__(self, cap):
        self._cap = cap

    def __getattr__(self, name):
        cap = self._cap

        def call(*args):
            if name == "hipEventCreateWithFlags":
                args[0]._obj.value = EV_BASE + cap.n_events
                cap.n_events += 1
                cap.log.append([name, "event#%d" % (cap.n_events - 1), args[1]])
            else:
                cap.record(name, args)
            return 0
        return call


def _plain(v):
    if isinstance(v, np.ndarray):
        if v.dtype.names:
            return {n: _plain(v[n]) for n in v.dtype.names}
        return [_plain(x) for x in v.tolist()]
    if isinstance(v, (np.floating, np.integer)):
        return v.item()
    if isinstance(v, float) and v != v:
        return "nan"
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in sorted(v.items())}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def _results(res):
    if res is None:
        return None
    if isinstance(res, E.BatchResult):
        return {"batch": [_plain(getattr(res, k)) for k in ("index", "value", "score",
                                                             "n_scored")]}
    out = []
    for r in res:
        row = [r.label, _plain(r.index), _plain(r.value), _plain(r.score), _plain(r.n_scored)]
        for k in ("below_llik", "above_llik", "cand"):
            v = getattr(r, k)
            row.append(None if v is None else [len(v), _sha(np.asarray(v).tobytes())])
        extra = {}
        for k, v in sorted(r.extra.items()):
            extra[k] = _sha(repr(_plain(v)).encode())
        row.append(extra)
        out.append(row)
    return out


# -- the levels -----------------------------------------------------------------
def c3_case(calls=5, run_kw=None, **knobs):
    """bench.py's C3 level as a WorkBatch: eager, eager, recorded, re-issued,
    then re-issued after one appended row (new counts)."""
    cap = Capture(hashed=True, **knobs)
    space = bench.c3_space()
    vals, losses = bench.c3_history(space)
    mat = bench.c3_matrix(space, vals)
    hist = cap.history(len(space), bench.T_HIST + 64)  # (room for the appended row)
    hist.append(mat)
    units = hdist.plan_units([k for _, k, _ in space], bench.N_CAND, 1)[0]
    out = []
    for k in range(calls):
        if k == 4:  # one more trial: the counts change
            row = mat[17][None]
            hist.append(row)
            mat = np.concatenate([mat, row])
            losses = np.append(losses, -9.0)
        rb = bench.below_rows(losses)
        isb = np.zeros(losses.size, np.uint8)
        isb[rb] = 1
        works = bench.history_batch(space, mat, hist, rb, k, bench.N_CAND, 0, units,
                                    bench.N_CAND)
        kw = dict(run_kw() if run_kw else {})
        out.append(cap.run(works, precision=32, history=hist, is_below=isb, defer=k % 2 == 1,
                           **kw))
    return out


SMALL = [("u", "uniform", (-5.0, 5.0)), ("lu", "loguniform", (-5.0, 0.0)),
         ("qu", "quniform", (0.0, 40.0, 2.0)), ("qlu", "qloguniform", (0.0, 4.0, 1.0)),
         ("n", "normal", (0.0, 2.0)), ("ln", "lognormal", (0.0, 1.0)),
         ("qn", "qnormal", (0.0, 5.0, 1.0)), ("qln", "qlognormal", (0.0, 1.0, 1.0)),
         ("r", "randint", (8,)), ("c", "categorical", ((0.2, 0.3, 0.5),))]


def _draws(space, T, seed):
    rng = np.random.RandomState(seed)
    cols = []
    for _, kind, a in space:
        if kind in ("uniform", "quniform"):
            v = rng.uniform(a[0], a[1], T)
        elif kind in ("loguniform", "qloguniform"):
            v = np.exp(rng.uniform(a[0], a[1], T))
        elif kind in ("normal", "qnormal"):
            v = rng.normal(a[0], a[1], T)
        elif kind in ("lognormal", "qlognormal"):
            v = np.exp(rng.normal(a[0], a[1], T))
        elif kind == "randint":
            v = rng.randint(0, a[0], T).astype(np.float64)
        else:
            v = rng.randint(0, len(a[0]), T).astype(np.float64)
        if kind.startswith("q"):
            v = np.round(v / a[2]) * a[2]
        cols.append(v)
    return np.stack(cols, axis=1)


def upload_works(space=SMALL, n_cand=24, inject=(), seed=3):
    mat = _draws(space, 25, seed)
    cands = _draws(space, 6, seed + 1)
    return [E.LabelWork(label=lab, kind=kind, args=a, obs_below=mat[:5, j], obs_above=mat[5:, j],
                        n_cand=n_cand, key=1000 + j, cand_base=3,
                        cand=cands[:, j] if lab in inject else None)
            for j, (lab, kind, a) in enumerate(space)]


def upload_case(space=SMALL, n_cand=24, inject=(), **kw):
    cap = Capture()
    return [cap.run(upload_works(space, n_cand, inject), **kw)]


def history_works(cap, space, T, seed, rows=None, hist_index=0, key0=0):
    """(history, works, is_below): a small history and its LabelWork list;
    ``rows``: the explicit row list the level reads."""
    mat = _draws(space, T, seed)
    hist = cap.history(len(space), 64)
    hist.append(mat)
    pos = np.arange(T) if rows is None else np.asarray(rows)
    isb = np.zeros(pos.size, np.uint8)
    isb[::5] = 1
    below = mat[pos[isb == 1]]
    works = [E.LabelWork(label=lab, kind=kind, args=a, obs_below=below[:, j], obs_above=None,
                         n_cand=24, key=key0 + j, cand_base=0, col=j,
                         n_above=int((isb == 0).sum()), hist=hist_index)
             for j, (lab, kind, a) in enumerate(space)]
    return hist, works, isb


def as_batch(name, works):
    return E.WorkBatch((name, len(works)), [np.size(w.obs_below) for w in works],
                       [w.n_above for w in works], [w.key for w in works],
                       [w.cand_base for w in works], lambda: works)


def rows_case():
    cap = Capture()
    rows = np.arange(1, 41, 2)
    hist, works, isb = history_works(cap, SMALL, 48, 5, rows=rows)
    return [cap.run(works, precision=32, history=hist, rows=rows, is_below=isb)
            for _ in range(3)]


def histories_case():
    cap = Capture()
    cap.pack_hash = False  # (the pack holds the histories' device addresses)
    h0, w0, isb0 = history_works(cap, SMALL, 40, 6)
    rows1 = np.arange(0, 30, 3)
    h1, w1, isb1 = history_works(cap, SMALL[:5], 36, 7, rows=rows1, hist_index=1, key0=50)
    hs = [(h0, None, isb0), (h1, rows1, isb1)]
    return [cap.run(as_batch("two-studies", w0 + w1), precision=32, histories=hs, defer=k == 1)
            for k in range(3)]


def exchange_case():
    cap = Capture()
    hist, works, isb = history_works(cap, SMALL, 40, 8)
    slots = np.arange(len(works), dtype=np.int32)[::-1].copy()
    return [cap.run(as_batch("shard", works), precision=32, history=hist, is_below=isb,
                    exchange=(COMM, len(works), 2, slots), defer=k == 1)
            for k in range(4)]


def _timers():
    return {"timers": {}}


def _timer_groups():
    return {"timers": {}, "timer_groups": {"fit", "table"}}


Q_FALLBACK = [("qfb", "quniform", (0.0, 1.0e7, 1.0)), ("u", "uniform", (0.0, 1.0))]
Q_WIDE = [("qw", "quniform", (0.0, 5000.0, 1.0)), ("q", "quniform", (0.0, 10.0, 1.0))]
Q_UNPACKED = [("qa", "quniform", (0.0, 70000.0, 1.0)), ("r", "randint", (4,))]

CASES = {
    "c3": lambda: c3_case(),
    "c3_side0": lambda: c3_case(side_stream="0"),
    "c3_side2": lambda: c3_case(side_stream="2"),
    "c3_cat_pre": lambda: c3_case(cat_issue="pre"),
    "c3_cat_late": lambda: c3_case(cat_issue="late"),
    "c3_cat_early_off": lambda: c3_case(cat_early=False),
    "c3_cat_hist_off": lambda: c3_case(cat_hist=False),
    "c3_sorted_fit_off": lambda: c3_case(sorted_fit=False),
    "c3_native_off": lambda: c3_case(native=False),
    "c3_poly": lambda: c3_case(table_scorer="poly"),
    "c3_lat_main_off": lambda: c3_case(lat_main=False),
    "c3_timers": lambda: c3_case(calls=4, run_kw=_timers),
    "c3_timer_groups": lambda: c3_case(calls=4, run_kw=_timer_groups),
    "history_rows": rows_case,
    "upload_fp64": lambda: upload_case(precision=64),
    "upload_fp32_outputs": lambda: upload_case(precision=32, outputs=True),
    "upload_fp32": lambda: upload_case(precision=32),
    "upload_injected": lambda: upload_case(inject=("u", "qu", "r"), precision=32),
    "upload_injected_fp64_outputs": lambda: upload_case(inject=("ln", "qln", "c"), precision=64,
                                                        outputs=True),
    "upload_dense": lambda: upload_case(precision=32, scorer="dense"),
    "upload_pruned_false": lambda: upload_case(precision=32, pruned=False),
    "upload_sorted": lambda: upload_case(precision=32, scorer="sorted"),
    "upload_table": lambda: upload_case(precision=32, scorer="table"),
    "upload_table_injected": lambda: upload_case(inject=("u", "n"), precision=32,
                                                 scorer="table"),
    "upload_sample_only": lambda: upload_case(precision=64, sample_only=True),
    "upload_posteriors": lambda: upload_case(precision=64, posteriors=True),
    "upload_table_scores": lambda: upload_case(precision=32, scorer="table", table_scores=True),
    "upload_prior_weight": lambda: upload_case(precision=32, prior_weight=0.5, lf=10),
    "lattice_fallback": lambda: upload_case(Q_FALLBACK, precision=32),
    "lattice_wide": lambda: upload_case(Q_WIDE, n_cand=1 << 17, precision=32),
    "lattice_unpacked": lambda: upload_case(Q_UNPACKED, precision=32),
    "quantized_main_stream": lambda: upload_case([SMALL[2], SMALL[8]], precision=32),
    "histories": histories_case,
    "exchange": exchange_case,
}


def capture(name):
    """The records of one case, as plain JSON values."""
    hip = L.hip
    try:
        return json.loads(json.dumps(CASES[name]()))
    finally:
        L.hip = hip  # (make_engine points it at its stand-in)


def dump(data):
    """One launch per line: a diff of two runs names the launch that moved."""
    lines = ["{"]
    for ci, (name, calls) in enumerate(data.items()):
        lines.append(" %s: [" % json.dumps(name))
        for k, call in enumerate(calls):
            lines.append("  {")
            lines.append('   "launches": [')
            rows = call["launches"]
            for i, row in enumerate(rows):
                lines.append("    " + json.dumps(row) + ("," if i + 1 < len(rows) else ""))
            lines.append("   ],")
            rest = [k2 for k2 in call if k2 != "launches"]
            for i, k2 in enumerate(rest):
                lines.append("   %s: %s%s" % (json.dumps(k2), json.dumps(call[k2], sort_keys=True),
                                              "," if i + 1 < len(rest) else ""))
            lines.append("  }" + ("," if k + 1 < len(calls) else ""))
        lines.append(" ]" + ("," if ci + 1 < len(data) else ""))
    lines.append("}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    text = dump({name: capture(name) for name in CASES})
    assert json.loads(text) is not None
    with open(path, "w") as f:
        f.write(text)
    print("%s: %d cases, %d bytes" % (path, len(CASES), len(text)))
