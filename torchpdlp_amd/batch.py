"""Batched solves: B LPs that share one constraint matrix and differ in c, q, l, u, advanced together in every launch.

``pdlp_algorithm_batch`` runs the reference's ``pdlp_algorithm`` (``/root/reference/PDLP/primal_dual_hybrid_gradient.py:7-181``) on
every LP of the batch at once.  A restart check only happens at ``t % restart_period == 0`` and ``t`` resets only at a restart,
which is always taken at a check (pdhg.py:115-146), so every LP's checks fall on multiples of ``restart_period`` of its iteration
count ``k``: checking all live LPs together every ``restart_period`` iterations runs each through exactly the reference's control
flow.  The step size, primal weight, restarts, KKT-pass count ``j`` and termination are per LP; a finished LP is frozen (its
column is never written again).  The kernels: ``pdlp_batch_*`` (include/pdlp_hip.h).
"""
from __future__ import annotations

import ctypes as C
import time
from typing import Optional

import numpy as np
import torch

from . import _native as N
from .engine import PdlpEngine
from .solver import (STATUS_KKT_LIMIT, STATUS_SOLVED, STATUS_TIME_LIMIT, _np_t, estimate_sigma, primal_weight_from_distances)
from .sparse import CsrPair

BETA = (0.2, 0.8, 0.36)                      # pdhg.py:28
_DT = {torch.float32: N.PDLP_F32, torch.float64: N.PDLP_F64}


def group_width(B: int, dtype) -> int:
    """W of the launches: the smallest of 8 / 16 / 32 that holds B, at most one 128-byte line of gathered values"""
    cap = 32 if dtype == torch.float32 else 16
    for w in (8, 16, 32):
        if B <= w or w == cap:
            return w
    return cap


def kkt_finish(red: np.ndarray, omega: np.ndarray, t=np.float32) -> dict:
    """helpers.py:84-106 per LP from the six sums of a KKT pass (``red`` [B, 6] in the order of PDLP_BUF_RED), in the working
    precision -- the vectorised form of the library's kkt_finish"""
    p, d, lp, un = (red[:, i].astype(t) for i in (3, 5, 1, 2))
    adj = (d + lp + un).astype(t)
    gap = (adj - p).astype(t)
    pr, dr = np.sqrt(red[:, 4]).astype(t), np.sqrt(red[:, 0]).astype(t)
    res = dict(pr=pr, dr=dr, gap=gap, p=p, d_adj=adj)
    res["kkt"] = kkt_reweight(res, omega, t)
    return res


def kkt_reweight(res: dict, omega: np.ndarray, t=np.float32) -> np.ndarray:
    """``kkt_from_residuals`` per LP: the KKT error of known residuals under omega (helpers.py:98-108, pdhg.py:153)"""
    w = np.asarray(omega).astype(t)
    w2 = (w * w).astype(t)
    pr, dr, gap = res["pr"], res["dr"], res["gap"]
    return np.sqrt((w2 * (pr * pr) + (dr * dr) / w2 + gap * gap).astype(t)).astype(t)


def termination(res: dict, q_norm, c_norm, tol, t=np.float32) -> np.ndarray:
    """``check_termination`` (helpers.py:110-128) per LP; the gap is signed (quirk Q2)"""
    tol, one = t(tol), t(1)
    c1 = res["pr"] <= tol * (one + q_norm)
    c2 = res["dr"] <= tol * (one + c_norm)
    c3 = res["gap"] <= tol * (one + np.abs(res["p"]) + np.abs(res["d_adj"]))
    return c1 & c2 & c3


def batch_decisions(kkt_cur, kkt_avg, kkt_prev, kkt_first, tt, k, j, live, max_kkt, t=np.float32) -> dict:
    """The restart decisions of one check (pdhg.py:115-146) and the KKT-pass cap (pdhg.py:54,67) per LP, over arrays.

    ``kkt_*`` are the KKT errors at the current, averaged and previous iterates, ``kkt_first`` the one of the last restart point
    (0 before the first restart: the first check can only restart artificially), ``tt`` the iterations since the last restart,
    ``k`` the iteration count, ``j`` the KKT-pass count AFTER the check's three passes.  Returns ``crit`` (-1 none, 0 sufficient,
    1 necessary, 2 artificial), ``use_avg``, ``capped`` (no restart, and ``j`` has reached ``max_kkt``: the reference leaves the
    inner loop and continues at pdhg.py:148 from the current iterate) and ``action`` (0 keep, 1 restart at the current iterate,
    2 at the average).  Dead LPs get -1 / False / 0."""
    kc, ka, kp, kf = (np.asarray(a, dtype=t) for a in (kkt_cur, kkt_avg, kkt_prev, kkt_first))
    live = np.asarray(live, dtype=bool)
    k_min = np.minimum(kc, ka)
    use_avg = (kc >= ka) & live
    suff = k_min <= t(BETA[0]) * kf
    nec = (k_min <= t(BETA[1]) * kf) & (k_min > kp)
    art = np.asarray(tt, dtype=np.float64) >= BETA[2] * np.asarray(k, dtype=np.float64)
    crit = np.where(suff, 0, np.where(nec, 1, np.where(art, 2, -1)))
    crit = np.where(live, crit, -1)
    restart = crit >= 0
    capped = live & ~restart & (np.asarray(j) >= max_kkt)
    action = np.where(restart, np.where(use_avg, 2, 1), np.where(capped, 1, 0))
    return dict(crit=crit, use_avg=use_avg, capped=capped, action=action.astype(np.int32))


class BatchEngine:
    """The device state of a batch: the populations ``[rows][Bp]`` and per-LP scalars that ``pdlp_batch_*`` work on, over the
    handle of a single-GPU ``PdlpEngine`` (its CSR arrays of K and K', its stream)."""

    def __init__(self, K: CsrPair, m_ineq: int, C_, Q, L, U, B: int, d_col=None, d_row=None, W: Optional[int] = None):
        dev, dt = K.val.device, K.val.dtype
        if dt not in _DT:
            raise ValueError(f"unsupported dtype {dt}")
        self.B, self.dtype, self.device = int(B), dt, dev
        self.W = int(W) if W is not None else group_width(self.B, dt)
        if self.W not in (8, 16, 32):
            raise ValueError("group width must be 8, 16 or 32")
        self.Bp = -(-self.B // self.W) * self.W
        self.m, self.n, self.m_ineq = K.m, K.n, int(m_ineq)
        first = lambda v: v if v.dim() == 1 else v[:, 0]
        self.eng = PdlpEngine(K.m, K.n, m_ineq, (K.rowptr, K.colidx, K.val), (K.t_rowptr, K.t_colidx, K.t_val),
                              first(C_), first(Q), first(L), first(U), d_col=d_col, d_row=d_row, tiles=False)
        self.lib, self.stream = self.eng.lib, self.eng.stream
        self.vec = [self._col(v, ln) for v, ln in ((C_, self.n), (Q, self.m), (L, self.n), (U, self.n))]
        e = lambda rows: torch.zeros(rows, self.Bp, dtype=dt, device=dev)
        self.x, self.x_prev, self.xbar, self.x_sum, self.x_avg, self.x_last = (e(self.n) for _ in range(6))
        self.y, self.y_prev, self.y_sum, self.y_avg, self.y_last, self.dy = (e(self.m) for _ in range(6))
        self.eta, self.omega, self.eta_sum, self.wpend = (torch.zeros(self.Bp, dtype=dt, device=dev) for _ in range(4))
        self.live = torch.zeros(self.Bp, dtype=torch.int32, device=dev)
        self.action = torch.zeros(self.Bp, dtype=torch.int32, device=dev)
        self.part = torch.zeros(N.BATCH_PART_PER_COL * self.Bp, dtype=torch.float64, device=dev)
        self.out = torch.zeros(3, self.Bp, 6, dtype=torch.float64, device=dev)
        p = lambda t: t.data_ptr()
        self.desc = N.PdlpBatch(self.B, self.Bp, self.W, *(int(v.dim() == 2) for v in self.vec), *(p(v) for v in self.vec),
                                p(self.x), p(self.x_prev), p(self.xbar), p(self.x_sum), p(self.x_avg), p(self.x_last),
                                p(self.y), p(self.y_prev), p(self.y_sum), p(self.y_avg), p(self.y_last), p(self.dy),
                                p(self.eta), p(self.omega), p(self.eta_sum), p(self.wpend), p(self.live), p(self.action),
                                p(self.part), p(self.out))

    def _col(self, v: torch.Tensor, ln: int) -> torch.Tensor:
        """a shared vector as it is, a per-LP one [len, B] padded to [len, Bp] (padding columns are dead)"""
        v = v.to(device=self.device, dtype=self.dtype)
        if v.dim() == 1:
            return v.contiguous()
        out = torch.zeros(ln, self.Bp, dtype=self.dtype, device=self.device)
        out[:, :v.shape[1]] = v
        return out

    def _pad(self, v: Optional[torch.Tensor], ln: int) -> torch.Tensor:
        out = torch.zeros(ln, self.Bp, dtype=self.dtype, device=self.device)
        if v is not None:
            v = v.to(device=self.device, dtype=self.dtype)
            out[:, :self.B] = v.reshape(-1, 1) if v.dim() == 1 else v
        return out

    def start(self, eta, omega, x_init=None, y_init=None):
        """pdhg.py:22-48 for every LP: the iterate (zeros or the given start), the restart point, empty sums, the step sizes"""
        with torch.cuda.stream(self.stream):
            self.x.copy_(self._pad(x_init, self.n))
            self.y.copy_(self._pad(y_init, self.m))
            self.x_last.copy_(self.x)
            self.y_last.copy_(self.y)
            for t in (self.x_sum, self.y_sum, self.eta_sum, self.wpend):
                t.zero_()
        live = np.zeros(self.Bp, np.int32)
        live[:self.B] = 1
        self.set_scalars(eta=eta, omega=omega, live=live)

    def set_scalars(self, **kw):
        """write per-LP arrays of the host ([B] or [Bp]) into the device scalars (stream-ordered)"""
        with torch.cuda.stream(self.stream):
            for name, v in kw.items():
                dst = getattr(self, name)
                v = np.asarray(v)
                full = np.zeros(self.Bp, dtype=v.dtype)
                full[:v.shape[0]] = v
                dst.copy_(torch.from_numpy(full).to(dst.dtype))

    def iterate(self, iters: int, adaptive: bool, k0: int):
        N.check(self.lib.pdlp_batch_iterate(self.eng.h, C.byref(self.desc), int(iters), int(adaptive), int(k0)), "pdlp_batch_iterate")

    def average(self, adaptive: bool):
        N.check(self.lib.pdlp_batch_average(self.eng.h, C.byref(self.desc), int(adaptive)), "pdlp_batch_average")

    def kkt(self, which: int, slot: int, unscaled: bool = False):
        N.check(self.lib.pdlp_batch_kkt(self.eng.h, C.byref(self.desc), int(which), int(unscaled), int(slot)), "pdlp_batch_kkt")

    def restart(self, slot: int):
        N.check(self.lib.pdlp_batch_restart(self.eng.h, C.byref(self.desc), int(slot)), "pdlp_batch_restart")

    def read_out(self) -> np.ndarray:
        """the [3][B][6] sums of the passes issued since the last read (synchronises the stream: one host read)"""
        with torch.cuda.stream(self.stream):
            return self.out[:, :self.B].cpu().numpy()

    def synchronize(self):
        self.stream.synchronize()


class BatchDriver:
    """``PdhgDriver``'s state machine (solver.py) vectorised over the LPs of a batch: numpy arrays of per-LP counters and scalars
    in the working precision, one host read per restart check (and one more when any LP restarts)."""

    def __init__(self, be: BatchEngine, q_norm, c_norm, restart_period=40, primal_update=False, adaptive=False, precondition=False,
                 tol=1e-4, max_kkt=100_000, traces=None):
        self.be, self.period = be, int(restart_period)
        self.primal_update, self.adaptive, self.precondition = bool(primal_update), bool(adaptive), bool(precondition)
        self.tol, self.max_kkt, self.traces = tol, int(max_kkt), traces
        self.t = t = _np_t(be.dtype)
        B = be.B
        self.q_norm, self.c_norm = np.asarray(q_norm, t), np.asarray(c_norm, t)
        self.k, self.n, self.j, self.tt = (np.zeros(B, np.int64) for _ in range(4))
        self.kkt_first = np.zeros(B, t)
        self.omega = np.ones(B, t)
        self.live = np.ones(B, bool)
        self.status = [STATUS_KKT_LIMIT] * B
        self.obj = np.full(B, np.nan)
        self.k_global = 0

    def start(self, sigma, x_init=None, y_init=None):
        t = self.t
        eta = t(0.9) / t(sigma)                                              # pdhg.py:22
        ok = (self.q_norm > 1e-6) & (self.c_norm > 1e-6)                     # pdhg.py:23
        with np.errstate(divide="ignore", invalid="ignore"):
            self.omega = np.where(ok, self.c_norm / self.q_norm, t(1.0)).astype(t)
        self.be.start(np.full(self.be.B, eta, t), self.omega, x_init, y_init)

    def _finish(self, idx, status):
        for i in idx:
            self.status[i] = status
        self.live[idx] = False

    def step(self, time_left: bool = True):
        """one segment: iterations up to the next check (or the first LP's KKT-pass cap), then the check and the restarts"""
        be, t, B = self.be, self.t, self.be.B
        live = self.live.copy()
        if not time_left:                                                    # pdhg.py:68-74, the global clock
            self._finish(np.flatnonzero(live), STATUS_TIME_LIMIT)
            return
        iters = min(self.period - self.k_global % self.period, int((self.max_kkt - self.j[live]).min()))
        if iters <= 0:                                                       # max_kkt <= 0: the reference's loop never runs
            self._finish(np.flatnonzero(live), STATUS_KKT_LIMIT)
            return
        be.iterate(iters, self.adaptive, self.k_global)                       # pdhg.py:76-112
        self.k_global += iters
        self.k[live] += iters
        self.j[live] += iters
        self.tt[live] += iters
        chosen = None
        if self.k_global % self.period == 0:                                 # pdhg.py:115 (tt = k mod period for every live LP)
            be.average(self.adaptive)                                        # pdhg.py:118-119
            for slot, which in enumerate((N.CUR, N.AVG, N.PREV)):           # pdhg.py:122-125
                be.kkt(which, slot)
            out = be.read_out()
            r = [kkt_finish(out[s], self.omega, t) for s in range(3)]
            self.j[live] += 3                                                 # pdhg.py:128
            dec = batch_decisions(r[0]["kkt"], r[1]["kkt"], r[2]["kkt"], self.kkt_first, self.tt, self.k, self.j, live,
                                  self.max_kkt, t)
            if self.traces is not None:
                for i in np.flatnonzero(live):
                    tr = self.traces[i]
                    tr["kkt"] += [float(r[0]["kkt"][i]), float(r[1]["kkt"][i]), float(r[2]["kkt"][i])]
                    if dec["crit"][i] >= 0:
                        tr["restarts"].append((int(dec["crit"][i]), int(self.tt[i]), int(dec["use_avg"][i])))
            chosen = {key: np.where(dec["use_avg"], r[1][key], r[0][key]) for key in r[0]}
            action, capped = dec["action"], dec["capped"]
        else:                                                                # only the cap ends an inner loop between checks
            capped = live & (self.j >= self.max_kkt)
            action = np.where(capped, 1, 0).astype(np.int32)
        act = np.flatnonzero(action)
        if act.size == 0:
            return
        # pdhg.py:133-165 for the LPs that leave their inner loop
        be.set_scalars(action=action)
        be.restart(0)
        if capped.any():           # no check chose their point: a pass at the current iterate (pdhg.py:153 after the cap)
            be.kkt(N.CUR, 2)
        if self.precondition:
            be.kkt(N.CUR, 1, unscaled=True)                                  # pdhg.py:157-163
        out = be.read_out()
        be.set_scalars(action=np.zeros(B, np.int32))
        self.n[act] += 1
        self.tt[act] = 0
        if self.primal_update:                                               # pdhg.py:150-151
            for i in act:
                self.omega[i] = primal_weight_from_distances(out[0, i, 0], out[0, i, 1], self.omega[i], 0.5, t)
            be.set_scalars(omega=self.omega)
            if self.traces is not None:
                for i in act:
                    self.traces[i]["omega"].append(float(self.omega[i]))
        if capped.any():
            rc = kkt_finish(out[2], self.omega, t)
            chosen = rc if chosen is None else {key: np.where(capped, rc[key], chosen[key]) for key in rc}
        kf = kkt_reweight(chosen, self.omega, t)                             # pdhg.py:153-154
        self.kkt_first[act] = kf[act]
        self.j[act] += 2                                                     # pdhg.py:154,165
        if self.traces is not None:
            for i in act:
                self.traces[i]["kkt"].append(float(kf[i]))
        res = kkt_finish(out[1], self.omega, t) if self.precondition else chosen
        self.obj[act] = res["p"][act].astype(np.float64)
        solved = termination(res, self.q_norm, self.c_norm, self.tol, t)     # pdhg.py:173
        done_s = act[solved[act]]
        done_k = act[~solved[act] & (self.j[act] >= self.max_kkt)]
        self._finish(done_s, STATUS_SOLVED)
        self._finish(done_k, STATUS_KKT_LIMIT)
        if done_s.size or done_k.size:
            be.set_scalars(live=self.live.astype(np.int32))                  # frozen from now on


def batch_size(*vecs) -> int:
    """B from the 2-D arguments (which must agree); 1 when every vector is shared"""
    bs = {int(v.shape[1]) for v in vecs if v is not None and v.dim() == 2}
    if len(bs) > 1:
        raise ValueError(f"the 2-D arguments disagree on the batch size: {sorted(bs)}")
    return bs.pop() if bs else 1


def pdlp_algorithm_batch(K, m_ineq, C_, Q, L, U, device=None, max_kkt=100_000, tol=1e-4, verbose=False, restart_period=40,
                         precondition=False, primal_update=False, adaptive=False, data_precond=None, time_limit=3600, time_used=0,
                         x_init=None, y_init=None, *, b0=None, sigma=None, seed=None, traces=None, group_width=None):
    """``pdlp_algorithm`` on B LPs with the same ``K`` at once.  ``C_``, ``Q``, ``L``, ``U``: 1-D (shared) or [len, B] (one column
    per LP), of the scaled problem when ``precondition`` (then ``data_precond`` = ``ruiz_precondition``'s: ``D_col``, ``D_row``
    give the un-scaled residuals).  ``traces``: a list of B dicts (``kkt``, ``omega``, ``restarts``) that receive every LP's trace.
    ``group_width``: W (8, 16, 32; default by B and dtype) -- results are bit-identical across batches of the same W.
    Returns ``(X, Y, obj, k, n, j, status, total_time)`` with X [n, B], Y [m, B] (the scaled iterates when preconditioned, like
    ``pdlp_algorithm``'s x) and numpy arrays / a list of status strings per LP."""
    t0 = time.time()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    Kp = CsrPair.from_any(K, device=device)
    B = batch_size(C_, Q, L, U)
    for name, v, ln in (("x_init", x_init, Kp.n), ("y_init", y_init, Kp.m)):
        if v is not None and (v.dim() not in (1, 2) or v.shape[0] != ln or (v.dim() == 2 and v.shape[1] != B)):
            raise ValueError(f"{name} must have shape ({ln},) or ({ln}, {B}), got {tuple(v.shape)}")
    d_col = d_row = None
    if precondition:
        if data_precond is None:
            raise ValueError("precondition=True needs data_precond from ruiz_precondition")
        d_col, d_row = data_precond[0], data_precond[1]
    be = BatchEngine(Kp, m_ineq, C_, Q, L, U, B, d_col=d_col, d_row=d_row, W=group_width)
    t = _np_t(Kp.dtype)
    # pdhg.py:19-20 per LP (as solver._global_norm: the float64 norm, rounded to the working precision)
    colnorm = lambda v: np.broadcast_to(np.sqrt((v.double().reshape(v.shape[0], -1) ** 2).sum(0).cpu().numpy()), (B,)).astype(t)
    qn, cn = colnorm(Q), colnorm(C_)
    if sigma is None:                                                        # pdhg.py:22: K only, once for the batch
        sigma = estimate_sigma(be.eng, b0, 100, seed)
    drv = BatchDriver(be, qn, cn, restart_period, primal_update, adaptive, precondition, tol, max_kkt, traces)
    drv.start(sigma, x_init, y_init)
    while drv.live.any():
        drv.step(time.time() - t0 + time_used < time_limit)
        if verbose:
            print(f"[batch] k={drv.k_global} live={int(drv.live.sum())}/{B}")
    be.synchronize()
    return (be.x[:, :B].clone(), be.y[:, :B].clone(), drv.obj, drv.k, drv.n, drv.j, list(drv.status), time.time() - t0 + time_used)
