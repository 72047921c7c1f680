"""Direct calls of the lattice exports (csrc/tpe_quantized.hip) for
tests/test_gpu_lattice_stages.py: tpe_lattice_sample, tpe_lattice_compact,
tpe_score_quantized (injected values, or compacted ones with firsts / counts),
tpe_lattice_suggest, and tpe_sample for the reference stream.

The mixtures are explicit ones prepared on the device as
hyperopt_amd.mixture._Mixture prepares its single segment
(tpe_mixture_prepare), here two segments per job (below, above) in one
component pool -- for a case of tests/lattice_cases.py the oracle's fits of
its history, so the oracle scores the same mixtures.  The helper owns every
buffer the exports write: slot_first with one sentinel word before and after
each job's range, vals, firsts, counts, partial, need, best, err and the
reach arrays.
"""
import ctypes

import numpy as np

from hyperopt_amd import _lib as L
from tests import lattice_cases as LC

_P = ctypes.c_void_p
SENTINEL = 0x5E5E5E5E5E5E5E5E
ONES = 0xFFFFFFFFFFFFFFFF
_FAM = {"GMM1": L.GMM1, "LGMM1": L.LGMM1}


def job_spec(c, draw=None, n_cand=None, cand_base=0, lattice=None):
    """A lattice_cases case as a Level job: the oracle's fits, the engine's
    lattice range and flags."""
    fam, pmu, psig, tf, low, high, q = LC.spec(c)
    kmin, n = LC.lattice(c) if lattice is None else lattice
    fb, fa = LC.fits(c)
    return dict(name=c.name, family=_FAM[fam], below=fb, above=fa, low=low, high=high, q=q,
                key=c.key, n_cand=c.n_cand if n_cand is None else n_cand, cand_base=cand_base,
                kmin=kmin, slots=n, flags=LC.job_flags(c, draw))


def mixture_spec(name, below, above, low, high, q, key, n_cand, kmin, slots, fp32, cand_base=0):
    """An explicit GMM1 pair (each (w, mu, sigma)) as a Level job."""
    flags = L.F_QUANT | ((L.F_LOW | L.F_HIGH) if low is not None else 0) | \
        (L.F_DRAW32 if fp32 else 0)
    return dict(name=name, family=L.GMM1, below=below, above=above, low=low, high=high, q=q,
                key=key, n_cand=n_cand, cand_base=cand_base, kmin=kmin, slots=slots, flags=flags)


class Level(object):
    """Several lattice jobs over explicit mixtures prepared on the device."""

    def __init__(self, specs):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", torch.cuda.current_device())
        self.lib = L.load()
        self.specs, self.nj = specs, len(specs)
        segs = np.zeros(2 * self.nj, L.SEG_DTYPE)
        ws, mus, sgs, off = [], [], [], 0
        for j, sp in enumerate(specs):
            for side, (w, mu, s) in enumerate((sp["below"], sp["above"])):
                w, mu, s = (np.asarray(a, np.float64) for a in (w, mu, s))
                assert np.all(np.diff(mu) >= 0)  # sorted by mean, as a fit is
                S, pos = segs[2 * j + side], int(np.argmax(s))
                S["comp_off"], S["n_obs"], S["family"] = off, w.size - 1, sp["family"]
                S["prior_pos"], S["prior_weight"] = pos, w[pos]
                S["prior_mu"], S["prior_sigma"] = mu[pos], s[pos]
                if sp["low"] is not None:
                    S["bounded"], S["low"], S["high"] = 1, sp["low"], sp["high"]
                S["given"] = 1
                ws.append(w), mus.append(mu), sgs.append(s)
                off += w.size
        self.K, kmax = off, max(w.size for w in ws)
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.d_segs = self._up(segs)
        self.d_w, self.d_mu, self.d_sigma = (
            torch.from_numpy(np.concatenate(a)).to(self.dev) for a in (ws, mus, sgs))
        self.d_cdf = torch.empty(self.K, **f64)
        self.d_c64 = torch.empty(4 * self.K, **f64)
        self.d_c32 = torch.empty(4 * self.K, dtype=torch.float32, device=self.dev)
        scratch = torch.empty(max(int(self.lib.tpe_mixture_scratch_bytes(2 * self.nj, kmax)), 8),
                              dtype=torch.uint8, device=self.dev)
        self.sp = _P(torch.cuda.current_stream(self.dev).cuda_stream)
        L.check(self.lib.tpe_mixture_prepare(
            self._p(self.d_segs), 2 * self.nj, kmax, self._p(scratch), self._p(self.d_w),
            self._p(self.d_mu), self._p(self.d_sigma), self._p(self.d_cdf), self._p(self.d_c64),
            self._p(self.d_c32), self.sp), "tpe_mixture_prepare")
        torch.cuda.synchronize()
        # jobs: slot ranges with a sentinel word on each side, outputs back to back
        jobs = self.jobs = np.zeros(self.nj, L.JOB_DTYPE)
        lat_off, out_off = 0, 0
        for j, sp in enumerate(specs):
            J = jobs[j]
            J["family"], J["flags"] = sp["family"], sp["flags"]
            J["below"], J["above"] = 2 * j, 2 * j + 1
            if sp["low"] is not None:
                J["low"], J["high"] = sp["low"], sp["high"]
            J["q"], J["key"], J["n_cand"] = sp["q"], sp["key"], sp["n_cand"]
            J["cand_base"] = sp["cand_base"]
            J["lat_off"], J["lat_kmin"], J["lat_n"] = lat_off + 1, sp["kmin"], sp["slots"]
            J["out_off"] = out_off
            lat_off += sp["slots"] + 2
            out_off += sp["n_cand"]
        self.n_slot_words, self.n_out = lat_off, out_off
        self.max_n = int(jobs["lat_n"].max())
        i64 = dict(dtype=torch.int64, device=self.dev)
        self.d_slot = torch.empty(lat_off, **i64)
        self.d_vals = torch.empty(lat_off, **f64)
        self.d_firsts = torch.empty(lat_off, **i64)
        self.d_counts = torch.zeros(self.nj, **i64)
        self.d_need = torch.empty(self.nj, dtype=torch.int32, device=self.dev)
        self.d_err = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.d_best = torch.empty(self.nj * L.BEST_DTYPE.itemsize, dtype=torch.uint8,
                                  device=self.dev)
        self.d_reach = torch.empty(2 * self.K, **f64)

    # ---- plumbing -------------------------------------------------------------------
    def _up(self, arr):
        return self.torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to(self.dev)

    @staticmethod
    def _p(t):
        return _P(t.data_ptr())

    def _jobs(self, ready=False, **cols):
        """(host jobs, device copy) with TPE_F_LATTICE_READY set or clear and
        columns replaced."""
        hj = self.jobs.copy()
        for k, v in cols.items():
            hj[k] = v
        hj["flags"] = (hj["flags"] & ~L.F_LATTICE_READY) | (L.F_LATTICE_READY if ready else 0)
        return hj, self._up(hj)

    def _reach(self, on):
        if not on:
            return None, None
        return _P(self.d_reach.data_ptr()), _P(self.d_reach.data_ptr() + 8 * self.K)

    def _partial(self, n):
        return self.torch.empty(max(n, 1) * L.BEST_DTYPE.itemsize, dtype=self.torch.uint8,
                                device=self.dev)

    def _fill_slots(self, ready):
        """The caller's part of the slot buffer: sentinels everywhere, and
        (ready) all-ones on every job's own range."""
        a = np.full(self.n_slot_words, SENTINEL, np.uint64)
        if ready:
            for J in self.jobs:
                a[J["lat_off"]:J["lat_off"] + J["lat_n"]] = ONES
        self.d_slot.copy_(self.torch.from_numpy(a.view(np.int64)))
        self.d_err.zero_()

    def read_slots(self, ready):
        """(per-job first-index tables as uint64, sentinels intact).  With the
        library's memset (ready clear) the words between the jobs belong to
        the cleared range [0, end): they must read all-ones -- a kernel's
        atomicMin would have lowered them -- and the word past the last job
        must still be the sentinel."""
        a = self.d_slot.cpu().numpy().view(np.uint64)
        tables, ok = [], True
        for j, J in enumerate(self.jobs):
            lo, n = int(J["lat_off"]), int(J["lat_n"])
            tables.append(a[lo:lo + n].copy())
            for pos in (lo - 1, lo + n):
                want = SENTINEL if ready or pos == self.n_slot_words - 1 else ONES
                ok = ok and int(a[pos]) == want
        return tables, ok

    def err(self):
        return int(self.d_err.item())

    # ---- the exports ----------------------------------------------------------------
    def stream(self, precision, quantized=True):
        """tpe_sample's candidates of every job, at one precision."""
        hj, dj = self._jobs()
        if not quantized:
            hj["flags"] &= ~L.F_QUANT
            dj = self._up(hj)
        out = self.torch.empty(max(self.n_out, 1), dtype=self.torch.float64, device=self.dev)
        L.check(self.lib.tpe_sample(self._p(dj), hj.ctypes.data_as(_P), self.nj,
                                    self._p(self.d_segs), self._p(self.d_mu),
                                    self._p(self.d_sigma), self._p(self.d_cdf), precision,
                                    self._p(out), self.sp), "tpe_sample")
        x = out.cpu().numpy()
        return [x[int(J["out_off"]):int(J["out_off"] + J["n_cand"])].copy() for J in self.jobs]

    def own_streams(self):
        """Each job's reference stream: tpe_sample at the job's own draw
        precision (fp32 with TPE_F_DRAW32, else fp64)."""
        want32 = [bool(J["flags"] & L.F_DRAW32) for J in self.jobs]
        s32 = self.stream(32) if any(want32) else None
        s64 = self.stream(64) if not all(want32) else None
        return [s32[j] if want32[j] else s64[j] for j in range(self.nj)]

    def sample(self, ready=False, only=None):
        """tpe_lattice_sample on all jobs, or on the jobs `only` (a launch of
        their own over the same buffers).  Returns read_slots()."""
        self._fill_slots(ready)
        hj, dj = self._jobs(ready)
        n = self.nj
        if only is not None:
            assert ready  # (the memset would run over the other jobs' ranges)
            hj = hj[list(only)].copy()
            dj, n = self._up(hj), len(hj)
        L.check(self.lib.tpe_lattice_sample(self._p(dj), hj.ctypes.data_as(_P), n,
                                            self._p(self.d_segs), self._p(self.d_mu),
                                            self._p(self.d_sigma), self._p(self.d_cdf),
                                            self._p(self.d_slot), self._p(self.d_err), self.sp),
                "tpe_lattice_sample")
        return self.read_slots(ready)

    def compact(self, ready=False):
        """tpe_lattice_compact on the slots as they stand: per job (vals,
        firsts) of its counts[j] entries."""
        hj, dj = self._jobs(ready)
        self.d_counts.zero_()  # (the caller's part with the flag set; the library's otherwise)
        L.check(self.lib.tpe_lattice_compact(self._p(dj), hj.ctypes.data_as(_P), self.nj,
                                             self._p(self.d_slot), self._p(self.d_vals),
                                             self._p(self.d_firsts), self._p(self.d_counts),
                                             self.sp), "tpe_lattice_compact")
        cnt = self.d_counts.cpu().numpy()
        v, f = self.d_vals.cpu().numpy(), self.d_firsts.cpu().numpy()
        return [(v[int(J["lat_off"]):int(J["lat_off"]) + int(c)].copy(),
                 f[int(J["lat_off"]):int(J["lat_off"]) + int(c)].copy())
                for J, c in zip(self.jobs, cnt)]

    def score_compacted(self, reach=True):
        """tpe_score_quantized on the compacted values (firsts / counts):
        (per job partial records of its counts[j] entries, best records)."""
        hj, dj = self._jobs()
        npart = int(self.lib.tpe_quantized_partials(hj.ctypes.data_as(_P), self.nj, self.max_n))
        part = self._partial(npart)
        rh, rl = self._reach(reach)
        L.check(self.lib.tpe_score_quantized(
            self._p(dj), hj.ctypes.data_as(_P), self.nj, self._p(self.d_segs), self._p(self.d_w),
            self._p(self.d_mu), self._p(self.d_sigma), self._p(self.d_vals),
            self._p(self.d_firsts), self._p(self.d_counts), self.max_n, None, None,
            self._p(part), npart, self._p(self.d_best), self._p(self.d_err), rh, rl, self.sp),
            "tpe_score_quantized")
        p = part.cpu().numpy().view(L.BEST_DTYPE).reshape(self.nj, -1)
        cnt = self.d_counts.cpu().numpy()
        return [p[j, :int(cnt[j])].copy() for j in range(self.nj)], self.best()

    def score_values(self, values, reach=True):
        """tpe_score_quantized on injected values (one array per job): per
        job (below log-mass, above log-mass, partial scores)."""
        vals = [np.ascontiguousarray(v, np.float64) for v in values]
        sizes = np.array([v.size for v in vals], np.int64)
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        hj, dj = self._jobs(n_cand=sizes, cand_off=offs, out_off=offs, cand_base=0)
        hj["flags"] |= L.F_INJECTED
        dj = self._up(hj)
        torch = self.torch
        d_x = torch.from_numpy(np.concatenate(vals)).to(self.dev)
        d_bl, d_al = torch.empty_like(d_x), torch.empty_like(d_x)
        mx = int(sizes.max())
        npart = int(self.lib.tpe_quantized_partials(hj.ctypes.data_as(_P), self.nj, mx))
        part = self._partial(npart)
        best = torch.empty(self.nj * L.BEST_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        err = torch.zeros(1, dtype=torch.int32, device=self.dev)
        rh, rl = self._reach(reach)
        L.check(self.lib.tpe_score_quantized(
            self._p(dj), hj.ctypes.data_as(_P), self.nj, self._p(self.d_segs), self._p(self.d_w),
            self._p(self.d_mu), self._p(self.d_sigma), self._p(d_x), None, None, mx,
            self._p(d_bl), self._p(d_al), self._p(part), npart, self._p(best), self._p(err), rh,
            rl, self.sp), "tpe_score_quantized")
        bl, al = d_bl.cpu().numpy(), d_al.cpu().numpy()
        p = part.cpu().numpy().view(L.BEST_DTYPE).reshape(self.nj, -1)
        return [(bl[o:o + n].copy(), al[o:o + n].copy(), p[j, :n]["score"].copy())
                for j, (o, n) in enumerate(zip(offs, sizes))], int(err.item())

    def suggest(self, prefix=LC.PREFIX, reach=True, ready=False):
        """tpe_lattice_suggest: dict(best, need, partial (the slot records per
        job), tables, sentinels)."""
        self._fill_slots(ready)
        hj, dj = self._jobs(ready)
        npart = self.nj * self.max_n
        part = self._partial(npart)
        part.fill_(0x7B)  # (a pattern no score_slots record holds)
        rh, rl = self._reach(reach)
        L.check(self.lib.tpe_lattice_suggest(
            self._p(dj), hj.ctypes.data_as(_P), self.nj, self._p(self.d_segs), self._p(self.d_w),
            self._p(self.d_mu), self._p(self.d_sigma), self._p(self.d_cdf), self._p(self.d_slot),
            prefix, self._p(part), npart, self._p(self.d_need), self._p(self.d_best),
            self._p(self.d_err), rh, rl, self.sp), "tpe_lattice_suggest")
        p = part.cpu().numpy().view(L.BEST_DTYPE).reshape(self.nj, self.max_n)
        tables, ok = self.read_slots(ready)
        return dict(best=self.best(), need=self.d_need.cpu().numpy().copy(),
                    partial=[p[j, :int(J["lat_n"])].copy() for j, J in enumerate(self.jobs)],
                    tables=tables, sentinels=ok)

    def best(self):
        return self.d_best.cpu().numpy().view(L.BEST_DTYPE).copy()

    def full_stream_best(self, reach=True, ready=False):
        """sample -> compact -> score: the best records of the full streams."""
        self.sample(ready)
        self.compact(ready)
        return self.score_compacted(reach)[1]

    def slot_values(self, j):
        J = self.jobs[j]
        return (int(J["lat_kmin"]) + np.arange(int(J["lat_n"]))).astype(np.float64) * float(J["q"])


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def expected_table(cand, q, kmin, slots, cand_base):
    """The first-index table of a stream of lattice values: cand_base + first
    occurrence of (kmin + s) q, all-ones for a value that does not occur;
    values off the lattice range are left out (and counted)."""
    k = np.rint(cand / q).astype(np.int64)
    assert np.all(k.astype(np.float64) * q == cand)
    s = k - kmin
    inside = (s >= 0) & (s < slots)
    t = np.full(slots, ONES, np.uint64)
    u, f = np.unique(s[inside], return_index=True)
    t[u] = (cand_base + np.flatnonzero(inside)[f]).astype(np.uint64)
    return t, int(np.sum(~inside))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def read_engine(eng, jobs):
    """The lattice buffers of an engine's last level that ran sample ->
    compact -> score (as band_util.read_work reads the band work): per job
    (slot_first, vals, firsts) by the plan's job records."""
    out = []
    cnt = eng._bufs["lat_cnt"][:8 * len(jobs)].cpu().numpy().view(np.int64)
    for j, J in enumerate(jobs):
        lo, n = 8 * int(J["lat_off"]), int(J["lat_n"])
        slot = eng._bufs["lat_slot"][lo:lo + 8 * n].cpu().numpy().view(np.uint64).copy()
        c = int(cnt[j])
        vals = eng._bufs["lat_vals"][lo:lo + 8 * c].cpu().numpy().view(np.float64).copy()
        firsts = eng._bufs["lat_first"][lo:lo + 8 * c].cpu().numpy().view(np.int64).copy()
        out.append((slot, vals, firsts))
    return out
