"""The Halpern mode of the batched driver on the host: BatchDriver(halpern=True) over a numpy stand-in for BatchEngine against the
straight-line statement of the method LP by LP (tests/test_halpern_host.py), the refusals before any device work, the default
path's call sequence against the one recorded before the mode existed, and the binding of the new entry point (no GPU)."""
import json
import os
import re

import numpy as np
import pytest
import torch

import torchpdlp_amd as tp
from oracle import oracle as orc
from tests.test_halpern_host import halpern_model
from torchpdlp_amd import _native as N
from torchpdlp_amd import rules
from torchpdlp_amd.batch import BatchDriver, pdlp_algorithm_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = os.path.join(ROOT, "tests", "golden", "batch_driver_calls.json")
T = np.float32


class OracleBatchEngine:
    """what batch.py uses of BatchEngine, in numpy: B columns, each advanced by its own oracle's fixed PDHG step -- averaged PDHG
    (iterate / average) and the Halpern iteration as HalpernOracleEngine runs it.  A KKT pass stores sums from which
    rules.kkt_from_sums returns the oracle's residuals exactly (squares of float32 numbers are exact in float64).  ``calls`` is
    the sequence of calls with their arguments."""

    def __init__(self, lps, pdhg=True):
        self.lps, self.B, self.pdhg = lps, len(lps), pdhg
        self.dtype, self.device = torch.float32, torch.device("cpu")
        self.n, self.m = lps[0].n, lps[0].m
        self.calls = []
        self.out = np.zeros((3, self.B, 6))

    def log(self, name, *args):
        plain = lambda v: v.tolist() if isinstance(v, np.ndarray) else v.item() if isinstance(v, np.generic) else v
        self.calls.append([name] + [plain(a) for a in args])

    def start(self, eta, omega, x_init=None, y_init=None):
        self.log("start", np.asarray(eta, np.float64), np.asarray(omega, np.float64))
        B = self.B
        self.eta, self.omega = np.broadcast_to(np.asarray(eta, T), (B,)).copy(), np.asarray(omega, T).copy()
        self.x, self.y = [np.zeros(self.n, T) for _ in range(B)], [np.zeros(self.m, T) for _ in range(B)]
        self.x_last, self.y_last = [v.copy() for v in self.x], [v.copy() for v in self.y]
        self.x_prev, self.y_prev = [v.copy() for v in self.x], [v.copy() for v in self.y]
        self.x_avg, self.y_avg = [None] * B, [None] * B
        self.x_sum, self.y_sum = [np.zeros(self.n, T) for _ in range(B)], [np.zeros(self.m, T) for _ in range(B)]
        self.eta_sum = np.zeros(B, T)
        self.live, self.action = np.ones(B, np.int32), np.zeros(B, np.int32)

    def set_scalars(self, **kw):
        for name in sorted(kw):
            v = np.asarray(kw[name])
            self.log("set_scalars", name, v.astype(np.float64) if v.dtype.kind == "f" else v)
            setattr(self, name, v.astype(getattr(self, name).dtype).copy())

    def halpern_iterate(self, iters, t_since):
        self.log("halpern_iterate", int(iters), np.asarray(t_since))
        for b in np.flatnonzero(self.live):
            o = self.lps[b]
            for it in range(int(iters)):
                a, w = rules.halpern_weights(int(t_since[b]) + it, self.dtype)
                xc, yc = o.step_fixed(self.x[b], self.y[b], self.eta[b], self.omega[b], 1.0)
                self.x[b] = a * (xc + (xc - self.x[b])) + w * self.x_last[b]
                self.y[b] = a * (T(2) * yc - self.y[b]) + w * self.y_last[b]
                self.x_avg[b], self.y_avg[b] = xc, yc

    def iterate(self, iters, adaptive, k0):
        assert self.pdhg and not adaptive, "a PDHG iteration"
        self.log("iterate", int(iters), bool(adaptive), int(k0))
        for b in np.flatnonzero(self.live):
            for _ in range(int(iters)):
                self.x_prev[b], self.y_prev[b] = self.x[b], self.y[b]
                self.x[b], self.y[b] = self.lps[b].step_fixed(self.x[b], self.y[b], self.eta[b], self.omega[b], 1.0)
                self.x_sum[b] = self.x_sum[b] + self.eta[b] * self.x[b]
                self.y_sum[b] = self.y_sum[b] + self.eta[b] * self.y[b]
                self.eta_sum[b] = self.eta_sum[b] + self.eta[b]

    def average(self, adaptive):
        assert self.pdhg, "an average"
        self.log("average", bool(adaptive))
        for b in np.flatnonzero(self.live):
            self.x_avg[b], self.y_avg[b] = self.x_sum[b] / self.eta_sum[b], self.y_sum[b] / self.eta_sum[b]

    def kkt(self, which, slot, unscaled=False):
        self.log("kkt", int(which), int(slot), bool(unscaled))
        X, Y = {N.CUR: (self.x, self.y), N.AVG: (self.x_avg, self.y_avg), N.PREV: (self.x_prev, self.y_prev)}[which]
        for b in np.flatnonzero(self.live):
            r = self.lps[b].kkt(X[b], Y[b], 1.0)
            self.out[slot, b] = [np.float64(r["dr"]) ** 2, 0.0, 0.0, np.float64(r["p"]), np.float64(r["pr"]) ** 2, np.float64(r["d_adj"])]

    def read_out(self):
        self.log("read_out")
        return self.out.copy()

    def restart(self, slot):
        self.log("restart", int(slot))
        for b in np.flatnonzero(self.action):
            if self.action[b] == 2:
                self.x[b], self.y[b] = self.x_avg[b].copy(), self.y_avg[b].copy()
            self.out[slot, b, 0] = float(np.sum((self.x_last[b] - self.x[b]).astype(np.float64) ** 2))
            self.out[slot, b, 1] = float(np.sum((self.y_last[b] - self.y[b]).astype(np.float64) ** 2))
            self.x_last[b], self.y_last[b] = self.x[b].copy(), self.y[b].copy()
            self.x_sum[b], self.y_sum[b], self.eta_sum[b] = np.zeros(self.n, T), np.zeros(self.m, T), T(0)

    def synchronize(self):
        pass


@pytest.fixture(scope="module", autouse=True)
def _one_thread():
    orc.set_threads(1)


def family(g, name, B=3, seed=0):
    """the golden LP and B - 1 copies with another c each"""
    a = g.group(name)
    rng = np.random.default_rng(seed)
    cs = [a["c"]] + [(a["c"] * (1 + 0.02 * rng.standard_normal(a["c"].size))).astype(T) for _ in range(1, B)]
    return [orc.OracleLP(a["m"], a["n"], a["m_ineq"], a["rowptr"], a["colidx"], a["val"], c, a["q"], a["l"], a["u"]) for c in cs]


def norms(lps):
    nrm = lambda v: T(np.sqrt(np.sum(v.astype(np.float64) ** 2)))
    return np.array([nrm(o.q) for o in lps], T), np.array([nrm(o.c) for o in lps], T)


def drive(lps, sigma, pw, traces=None, max_kkt=100_000, **kw):
    be = OracleBatchEngine(lps, pdhg=not kw.get("halpern"))
    qn, cn = norms(lps)
    drv = BatchDriver(be, qn, cn, 40, primal_update=pw, tol=1e-4, max_kkt=max_kkt, traces=traces, **kw)
    drv.start(sigma)
    while drv.live.any():
        drv.step(True)
    return be, drv


@pytest.mark.parametrize("name", ["mixed_27x32", "mixed_400x300"])
@pytest.mark.parametrize("pw", [False, True], ids=["nopw", "pw"])
def test_batch_driver_runs_the_method_as_stated(golden, name, pw):
    g = golden("solve_trace.npz")
    lps = family(g, name)
    sigma = float(g.group(f"{name}/fixed_nopw")["sigma"])
    traces = [dict(kkt=[], omega=[], restarts=[]) for _ in lps]
    be, drv = drive(lps, sigma, pw, traces, halpern=True)
    for b, o in enumerate(lps):
        xm, km, nm, jm, restarts, sm = halpern_model(o, sigma, 1e-4, pw)
        assert (int(drv.k[b]), int(drv.n[b]), int(drv.j[b]), drv.status[b]) == (km, nm, jm, sm), b
        assert traces[b]["restarts"] == restarts, b
        assert np.array_equal(be.x[b], xm), b
        checks = km // 40
        assert jm == km + checks + 2 * nm and len(traces[b]["kkt"]) == 3 * checks + nm, b
        assert np.isinf(traces[b]["kkt"][0]) and np.isinf(traces[b]["kkt"][2]), b      # kkt_cur, and kkt_prev of a first check
        assert len(traces[b]["omega"]) == (nm if pw else 0), b
    assert drv.status[0] == "Solved"
    names = {c[0] for c in be.calls}
    assert "halpern_iterate" in names and not names & {"iterate", "average"}            # (the stand-in raises on either as well)
    # one pass per check, at the candidate; the passes after a restart at the current iterate
    assert all(c[1:3] in ([N.AVG, 1], [N.CUR, 2], [N.CUR, 1]) for c in be.calls if c[0] == "kkt")
    assert sum(c[1] for c in be.calls if c[0] == "halpern_iterate") == int(drv.k.max())
    # t_since of every call: each live LP's count since its restart, before the call
    assert all(len(c[2]) == len(lps) and min(c[2]) >= 0 for c in be.calls if c[0] == "halpern_iterate")


def test_a_capped_lp_keeps_its_candidate(golden):
    """max_kkt reached between two checks: the LP adopts the candidate of its last iteration (action 2), counts one more restart
    and two more passes, like run_pdlp"""
    g = golden("solve_trace.npz")
    lps = family(g, "mixed_27x32", B=2)
    sigma = float(g.group("mixed_27x32/fixed_nopw")["sigma"])
    be, drv = drive(lps, sigma, False, max_kkt=50, halpern=True)
    assert drv.status == [rules.STATUS_KKT_LIMIT] * 2
    assert drv.k.tolist() == [47, 47] and drv.n.tolist() == [2, 2] and drv.j.tolist() == [52, 52]
    i = max(i for i, c in enumerate(be.calls) if c[0] == "restart")
    assert be.calls[i - 1] == ["set_scalars", "action", [2, 2]]
    for b in range(2):
        assert np.array_equal(be.x[b], be.x_avg[b]) and np.array_equal(be.y[b], be.y_avg[b])
        assert (be.x[b] >= lps[b].l).all() and (be.x[b] <= lps[b].u).all()
    # the clock: live LPs between restarts adopt their candidate, no counter moves
    be = OracleBatchEngine(lps, pdhg=False)
    drv = BatchDriver(be, *norms(lps), 40, halpern=True)
    drv.start(sigma)
    drv.step(False)
    assert drv.status == [rules.STATUS_TIME_LIMIT] * 2 and not drv.k.any() and "restart" not in {c[0] for c in be.calls}
    be = OracleBatchEngine(lps, pdhg=False)
    drv = BatchDriver(be, *norms(lps), 40, halpern=True, max_kkt=30)
    drv.start(sigma)
    drv.step(True)
    drv.live[:] = True                       # (a cap that the clock overtakes: 30 iterations done, nothing adopted yet)
    drv.tt[:] = 30
    before = (drv.k.copy(), drv.n.copy(), drv.j.copy())
    drv.step(False)
    assert drv.status == [rules.STATUS_TIME_LIMIT] * 2
    assert all(np.array_equal(a, b) for a, b in zip(before, (drv.k, drv.n, drv.j)))
    assert [c for c in be.calls if c[0] == "set_scalars" and c[1] == "action"][-2][2] == [2, 2]


def test_refused_combination_raises_before_any_device_work(monkeypatch):
    f = tp.gen_lp_family(30, 20, 3, 3, seed=1)
    K = tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val)
    prob = (f.C[:, 0], K, f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0])
    monkeypatch.setattr(tp.batch, "BatchEngine", None)          # any device work would fail differently
    with pytest.raises(ValueError, match="halpern"):
        tp.solve_lp_batch(prob, f.C, device="cpu", halpern=True, adaptive_stepsize=True)
    with pytest.raises(ValueError, match="halpern"):
        pdlp_algorithm_batch(K, f.m_ineq, f.C, f.Q, f.L, f.U, "cpu", halpern=True, adaptive=True)
    with pytest.raises(ValueError, match="halpern"):
        BatchDriver(None, np.ones(3, T), np.ones(3, T), adaptive=True, halpern=True)
    # the flags without a batched form raise as they did, with the new keyword beside them
    for flag in (dict(infeasibility_detect=True), dict(adaptive_retry=True), dict(precision="mixed"), dict(comm=True)):
        with pytest.raises(ValueError, match="batched form"):
            tp.solve_lp_batch(prob, f.C, device="cpu", halpern=True, **flag)
    with pytest.raises(TypeError, match="unexpected keyword"):
        tp.solve_lp_batch(prob, f.C, device="cpu", halpern=True, halpern_restart="fixed_point")


@pytest.mark.parametrize("pw", [False, True], ids=["nopw", "pw"])
def test_default_call_sequence_is_the_recorded_one(golden, pw):
    """halpern=False (and no keyword at all): the calls the driver makes on the stand-in, with their arguments, are those recorded
    from the driver before the Halpern mode existed (tests/golden/batch_driver_calls.json: mixed_27x32, three columns, with a
    KKT-pass cap that one column reaches between two checks)"""
    g = golden("solve_trace.npz")
    lps = family(g, "mixed_27x32")
    sigma = float(g.group("mixed_27x32/fixed_nopw")["sigma"])
    want = json.load(open(CALLS))["pw" if pw else "nopw"]
    for kw in ({}, dict(halpern=False)):
        be, drv = drive(lps, sigma, pw, max_kkt=want["max_kkt"], **kw)
        assert json.loads(json.dumps(be.calls)) == want["calls"]
        assert [drv.k.tolist(), drv.n.tolist(), drv.j.tolist(), drv.status] == want["result"]
    assert not any(c[0] == "halpern_iterate" for c in want["calls"])


def test_binding_declares_the_entry_point_with_the_headers_signature():
    import ctypes as C
    src = open(os.path.join(ROOT, "include", "pdlp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"int\s+pdlp_batch_halpern_iterate\s*\(([^)]*)\)\s*;", src).group(1)
    assert [" ".join(a.split()) for a in decl.split(",")] == ["pdlp_handle h", "const pdlp_batch* b", "int iters", "const int64_t* t_since"]
    res, args = N.SIGNATURES["pdlp_batch_halpern_iterate"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(N.PdlpBatch), C.c_int, C.c_void_p]
    assert N.ABI_VERSION == 18
    lib = N.load()
    b = N.PdlpBatch()
    assert lib.pdlp_abi_version() == 18
    assert lib.pdlp_batch_halpern_iterate(None, C.byref(b), 1, None) == -1
    assert lib.pdlp_batch_halpern_iterate(None, C.byref(b), -1, None) == -1
    assert lib.pdlp_batch_halpern_iterate(None, None, 0, None) == -1
