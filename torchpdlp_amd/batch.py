"""Batched solves: B LPs that share one constraint matrix (or one sparsity pattern, each with its own values: ``K_values``) and
differ in c, q, l, u, advanced together in every launch.

``pdlp_algorithm_batch`` runs the reference's ``pdlp_algorithm`` (``/root/reference/PDLP/primal_dual_hybrid_gradient.py:7-181``) on
every LP of the batch at once.  A restart check only happens at ``t % restart_period == 0`` and ``t`` resets only at a restart,
which is always taken at a check (pdhg.py:115-146), so every LP's checks fall on multiples of ``restart_period`` of its iteration
count ``k``: checking all live LPs together every ``restart_period`` iterations runs each through exactly the reference's control
flow.  The step size, primal weight, restarts, KKT-pass count ``j`` and termination are per LP; a finished LP is frozen (its
column is never written again).  The kernels: ``pdlp_batch_*`` (include/pdlp_hip.h).

A family longer than the batch is wide is streamed (``slots``, ``_solve_stream``): a finished LP's column is retired and given to
the next LP of the family at a check, which by the same argument runs the control flow -- and gets the bits -- of the plain batch.
"""
from __future__ import annotations

import ctypes as C
import time
from typing import Optional

import numpy as np
import torch

from . import _native as N
from .engine import PdlpEngine
from .rules import (STATUS_KKT_LIMIT, STATUS_SOLVED, STATUS_TIME_LIMIT, StreamQueue, kkt_error, kkt_from_sums, np_type,
                    primal_weight, restart_decision, start_eta, start_omega, terminated)
from .solver import estimate_sigma, power_iteration_start, precond_factors, resolve_device
from .sparse import CsrPair

batch_decisions, kkt_finish, termination = restart_decision, kkt_from_sums, terminated      # (their earlier names)
HALPERN_BATCH_REFUSED = ("halpern=True runs the fixed step of every LP of a batch: not with adaptive (adaptive_stepsize)")
_DT = {torch.float32: N.PDLP_F32, torch.float64: N.PDLP_F64}


def group_width(B: int, dtype) -> int:
    """W of the launches: the smallest of 8 / 16 / 32 that holds B, at most one 128-byte line of gathered values"""
    cap = 32 if dtype == torch.float32 else 16
    for w in (8, 16, 32):
        if B <= w or w == cap:
            return w
    return cap


class BatchEngine:
    """The device state of a batch: the populations ``[rows][Bp]`` and per-LP scalars that ``pdlp_batch_*`` work on, over the
    handle of a single-GPU ``PdlpEngine`` (its CSR arrays of K and K', its stream)."""

    def __init__(self, K: CsrPair, m_ineq: int, C_, Q, L, U, B: int, d_col=None, d_row=None, W: Optional[int] = None,
                 K_values=None, KT_values=None):
        """``K_values`` ``(nnz, B)``: a matrix per LP over K's pattern, in the order of ``K.val`` (``KT_values``: the same values
        in the order of ``K.t_val``; default ``K_values[K.transpose_perm()]``); ``d_col`` / ``d_row`` are then ``(n, B)`` /
        ``(m, B)``, the Ruiz factors of every LP's own matrix."""
        dev, dt = K.val.device, K.val.dtype
        if dt not in _DT:
            raise ValueError(f"unsupported dtype {dt}")
        self.B, self.dtype, self.device = int(B), dt, dev
        self.W = int(W) if W is not None else group_width(self.B, dt)
        if self.W not in (8, 16, 32):
            raise ValueError("group width must be 8, 16 or 32")
        self.Bp = -(-self.B // self.W) * self.W
        self.m, self.n, self.m_ineq = K.m, K.n, int(m_ineq)
        first = lambda v: v if v is None or v.dim() == 1 or v.shape[1] == 1 else v[:, 0]
        self.eng = PdlpEngine(K.m, K.n, m_ineq, (K.rowptr, K.colidx, K.val), (K.t_rowptr, K.t_colidx, K.t_val),
                              first(C_), first(Q), first(L), first(U), d_col=first(d_col), d_row=first(d_row), tiles=False)
        self.lib, self.stream = self.eng.lib, self.eng.stream
        self.per_lp_matrices = K_values is not None
        # the un-scaling factors as columns: [len, 1] shared, [len, B] with a matrix per LP
        self.d_col, self.d_row = (None if d is None else d.to(device=dev, dtype=dt).reshape(d.shape[0], -1) for d in (d_col, d_row))
        if self.per_lp_matrices:
            if tuple(K_values.shape) != (K.nnz, self.B):
                raise ValueError(f"K_values must have shape ({K.nnz}, {self.B}), got {tuple(K_values.shape)}")
            # the caller's tensor serves as the population when it already is one ([nnz, Bp], contiguous, on the device); K' is
            # one gather of the padded K population: beside the caller's tensor at most two populations ever exist
            self.K_valB = self._population(K_values, K.nnz)
            self.KT_valB = self.K_valB[K.transpose_perm()] if KT_values is None else self._population(KT_values, K.nnz)
            fac = [None, None]
            if self.d_col is not None:
                if self.d_col.shape[1] != self.B or self.d_row.shape[1] != self.B:
                    raise ValueError("with K_values, d_col and d_row hold one column per LP")
                fac = self.d_colB, self.d_rowB = self._pad(self.d_col, self.n), self._pad(self.d_row, self.m)
            N.check(self.lib.pdlp_batch_attach_matrices(self.eng.h, self.Bp, self.K_valB.data_ptr(), self.KT_valB.data_ptr(),
                                                        *(None if f is None else f.data_ptr() for f in fac)),
                    "pdlp_batch_attach_matrices")
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
        self.k_start = None        # [Bp] int64 once the batch streams a family (enable_stream): the count at each column's admission
        self.t_since = None        # [Bp] int64 once the batch runs the Halpern iteration (halpern_iterate)

    def _pad(self, v: Optional[torch.Tensor], ln: int) -> torch.Tensor:
        """a fresh population [ln, Bp]: ``v`` [ln, B] in the columns of the LPs (1-D: the same in each; None: zeros), padding zero"""
        out = torch.zeros(ln, self.Bp, dtype=self.dtype, device=self.device)
        if v is not None:
            v = v.to(device=self.device, dtype=self.dtype)
            out[:, :self.B] = v.reshape(-1, 1) if v.dim() == 1 else v
        return out

    def _col(self, v: torch.Tensor, ln: int) -> torch.Tensor:
        """a shared vector as it is, a per-LP one [len, B] padded to [len, Bp] (padding columns are dead)"""
        return v.to(device=self.device, dtype=self.dtype).contiguous() if v.dim() == 1 else self._pad(v, ln)

    def _population(self, v: torch.Tensor, ln: int) -> torch.Tensor:
        """[ln, B] values as a population [ln, Bp]: ``v`` itself when it already is one, else a padded copy"""
        if v.device == self.device and v.dtype == self.dtype and tuple(v.shape) == (ln, self.Bp) and v.is_contiguous():
            return v
        return self._pad(v, ln)

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
        if self.k_start is not None:
            N.check(self.lib.pdlp_batch_iterate_from(self.eng.h, C.byref(self.desc), int(iters), int(adaptive), int(k0),
                                                     self.k_start.data_ptr()), "pdlp_batch_iterate_from")
            return
        N.check(self.lib.pdlp_batch_iterate(self.eng.h, C.byref(self.desc), int(iters), int(adaptive), int(k0)), "pdlp_batch_iterate")

    def halpern_iterate(self, iters: int, t_since):
        """``pdlp_batch_halpern_iterate``: ``iters`` iterations of the restarted, reflected Halpern iteration of every live LP, no
        host synchronisation.  ``t_since`` ([B] or [Bp] host integers): every LP's iterations since its last restart before the
        call.  Afterwards ``N.CUR`` is the Halpern iterate and ``N.AVG`` the candidate, one fixed PDHG step from it."""
        if self.t_since is None:
            self.t_since = torch.zeros(self.Bp, dtype=torch.int64, device=self.device)
        self.set_scalars(t_since=np.asarray(t_since, np.int64))
        N.check(self.lib.pdlp_batch_halpern_iterate(self.eng.h, C.byref(self.desc), int(iters), self.t_since.data_ptr()),
                "pdlp_batch_halpern_iterate")

    def enable_stream(self):
        """the state of a batch whose columns change hands (``admit`` / ``retire``): ``k_start``, and sums of its own for the
        retirements (``retire_out`` [3][Bp][6]: the KKT passes of the next check must not overwrite what no host read has fetched)"""
        self.k_start = torch.zeros(self.Bp, dtype=torch.int64, device=self.device)
        self.retire_out = torch.zeros(3, self.Bp, 6, dtype=torch.float64, device=self.device)
        self.retire_desc = N.PdlpBatch.from_buffer_copy(self.desc)
        self.retire_desc.out = self.retire_out.data_ptr()

    def _index(self, v) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(self.device)

    def admit(self, cols, ids, eta, omega, c=None, q=None, l=None, u=None, x0=None, y0=None, K_val=None, KT_val=None):
        """``pdlp_batch_admit``: column ``cols[i]`` starts on column ``ids[i]`` of the feed -- ``[len, N]`` device tensors of the
        working precision (None: the batch shares the vector / zeros / no matrices), ``eta`` and ``omega`` ``[N]`` host arrays"""
        Nf = {int(v.shape[1]) for v in (c, q, l, u, x0, y0, K_val, KT_val) if v is not None} | {int(np.shape(eta)[0]), int(np.shape(omega)[0])}
        if len(Nf) != 1:
            raise ValueError(f"the arrays of a feed disagree on its width: {sorted(Nf)}")
        for v in (c, q, l, u, x0, y0, K_val, KT_val):
            if v is not None and (v.dtype != self.dtype or v.device != self.device or not v.is_contiguous()):
                raise ValueError(f"a feed holds contiguous {self.dtype} tensors on {self.device}")
        with torch.cuda.stream(self.stream):
            sc = [torch.from_numpy(np.array(v)).to(device=self.device, dtype=self.dtype) for v in (eta, omega)]
            ct, it = self._index(cols), self._index(ids)
            p = lambda v: None if v is None else v.data_ptr()
            feed = N.PdlpBatchFeed(Nf.pop(), p(c), p(q), p(l), p(u), p(x0), p(y0), p(K_val), p(KT_val), p(sc[0]), p(sc[1]))
            N.check(self.lib.pdlp_batch_admit(self.eng.h, C.byref(self.desc), int(ct.numel()), ct.data_ptr(), it.data_ptr(), C.byref(feed)),
                    "pdlp_batch_admit")

    def retire(self, cols, ids, X_out, Y_out, rc_out=None, act_out=None, which: int = N.CUR, unscaled: bool = False, slot: int = 0):
        """``pdlp_batch_retire``: the solution report of ``cols`` into column ``ids[i]`` of the ``[len, N]`` result tensors; the six
        sums into ``retire_out[slot][cols[i]]`` (``out`` of a batch that does not stream).  No host read."""
        Nr = int(X_out.shape[1])
        for v, ln in ((X_out, self.n), (Y_out, self.m), (rc_out, self.n), (act_out, self.m)):
            if v is not None and (tuple(v.shape) != (ln, Nr) or v.dtype != self.dtype or v.device != self.device or not v.is_contiguous()):
                raise ValueError(f"a result array is a contiguous ({ln}, {Nr}) tensor of {self.dtype} on {self.device}")
        desc = self.retire_desc if self.k_start is not None else self.desc
        with torch.cuda.stream(self.stream):
            ct, it = self._index(cols), self._index(ids)
            p = lambda v: None if v is None else v.data_ptr()
            N.check(self.lib.pdlp_batch_retire(self.eng.h, C.byref(desc), int(ct.numel()), ct.data_ptr(), it.data_ptr(), int(which),
                                               int(bool(unscaled)), int(slot), p(X_out), p(Y_out), p(rc_out), p(act_out), Nr),
                    "pdlp_batch_retire")

    def average(self, adaptive: bool):
        N.check(self.lib.pdlp_batch_average(self.eng.h, C.byref(self.desc), int(adaptive)), "pdlp_batch_average")

    def kkt(self, which: int, slot: int, unscaled: bool = False):
        N.check(self.lib.pdlp_batch_kkt(self.eng.h, C.byref(self.desc), int(which), int(unscaled), int(slot)), "pdlp_batch_kkt")

    def report(self, which: int = N.CUR, unscaled: bool = False, slot: int = 0):
        """``pdlp_batch_report``: (reduced costs [n, B], row activities [m, B], the six sums [B, 6]) of EVERY LP, frozen or not
        (one host read)"""
        rc = torch.zeros(self.n, self.Bp, dtype=self.dtype, device=self.device)
        act = torch.zeros(self.m, self.Bp, dtype=self.dtype, device=self.device)
        with torch.cuda.stream(self.stream):
            N.check(self.lib.pdlp_batch_report(self.eng.h, C.byref(self.desc), int(which), int(bool(unscaled)), int(slot),
                                               rc.data_ptr(), act.data_ptr()), "pdlp_batch_report")
        return rc[:, :self.B], act[:, :self.B], self.read_out()[slot]

    def product(self, V: torch.Tensor, transpose: bool = False) -> torch.Tensor:
        """``pdlp_batch_product``: K V (V ``[n, Bp]`` -> ``[m, Bp]``) or K'V per column b < B, with every LP's own matrix when the
        batch has them; padding columns of the result are zero"""
        rows_in, rows_out = (self.m, self.n) if transpose else (self.n, self.m)
        if tuple(V.shape) != (rows_in, self.Bp) or V.dtype != self.dtype or not V.is_contiguous():
            raise ValueError(f"the population must be a contiguous ({rows_in}, {self.Bp}) tensor of {self.dtype}")
        out = torch.zeros(rows_out, self.Bp, dtype=self.dtype, device=self.device)
        with torch.cuda.stream(self.stream):
            N.check(self.lib.pdlp_batch_product(self.eng.h, C.byref(self.desc), int(bool(transpose)), V.data_ptr(), out.data_ptr()),
                    "pdlp_batch_product")
        return out

    def power_iteration(self, b0: torch.Tensor, iters: int = 100) -> np.ndarray:
        """spectral_norm_estimate_torch (helpers.py:41-51) on every LP's matrix at once, the same start vector for each: [B]"""
        with torch.cuda.stream(self.stream):
            V = self._pad(b0.reshape(-1), self.n)
            for _ in range(int(iters)):                                      # helpers.py:48-50
                V = self.product(self.product(V), transpose=True)
                V[:, :self.B] /= torch.linalg.vector_norm(V[:, :self.B], dim=0, keepdim=True)
            s = torch.linalg.vector_norm(self.product(V)[:, :self.B], dim=0)  # helpers.py:51
        s = s.double().cpu().numpy()
        if not (np.isfinite(s) & (s > 0)).all():          # K_b'K_b b = 0 on the way (0 / 0): the start step would be NaN
            bad = np.flatnonzero(~(np.isfinite(s) & (s > 0))).tolist()
            raise ValueError(f"the power iteration found no norm for the matrices of LPs {bad} (all entries zero?)")
        return s

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
    in the working precision, one host read per restart check (and one more when any LP restarts).

    ``halpern=True``: the restarted, reflected Halpern iteration per LP with ``PdhgDriver``'s rules.  A
    segment is ``be.halpern_iterate``; a check is ONE KKT pass at the candidate ``N.AVG`` and hands ``restart_decision``
    ``inf``, the candidate's KKT error and the candidate's error at the previous check of the LP's restart period (``inf`` at the
    first); a restart -- or the KKT-pass cap, or the clock, between restarts -- adopts the candidate (action 2).  KKT passes per
    LP: the iterations, 1 per check, 2 per restart."""

    def __init__(self, be: BatchEngine, q_norm, c_norm, restart_period=40, primal_update=False, adaptive=False, precondition=False,
                 tol=1e-4, max_kkt=100_000, traces=None, halpern=False):
        self.be, self.period = be, int(restart_period)
        self.halpern = bool(halpern)
        if self.halpern and adaptive:
            raise ValueError(HALPERN_BATCH_REFUSED)
        self.primal_update, self.adaptive, self.precondition = bool(primal_update), bool(adaptive), bool(precondition)
        self.tol, self.max_kkt, self.traces = tol, int(max_kkt), traces
        self.t = t = np_type(be.dtype)
        B = be.B
        self.q_norm, self.c_norm = np.asarray(q_norm, t), np.asarray(c_norm, t)
        self.k, self.n, self.j, self.tt = (np.zeros(B, np.int64) for _ in range(4))
        self.kkt_first = np.zeros(B, t)
        self.k_prev_cand = np.full(B, np.inf, t)        # Halpern: the candidate's KKT error at the previous check of the period
        self.omega = np.ones(B, t)
        self.live = np.ones(B, bool)
        self.status = [STATUS_KKT_LIMIT] * B
        self.obj = np.full(B, np.nan)
        self.lp = np.arange(B)               # column -> LP (the index into ``traces``); a streamed family changes it (occupy)
        self.k_global = 0

    def start(self, sigma, x_init=None, y_init=None):
        eta, self.omega = start_scalars(sigma, self.q_norm, self.c_norm, self.t)
        self.be.start(eta, self.omega, x_init, y_init)

    def occupy(self, cols, ids, q_norm, c_norm, omega):
        """columns ``cols`` start on LPs ``ids`` (pdhg.py:19-23,45-54 for each): their counters, norms, primal weight and status"""
        self.lp[cols] = ids
        self.q_norm[cols], self.c_norm[cols], self.omega[cols] = q_norm, c_norm, omega
        for a in (self.k, self.n, self.j, self.tt, self.kkt_first):
            a[cols] = 0
        self.k_prev_cand[cols] = np.inf
        self.obj[cols] = np.nan
        self.live[cols] = True
        for i in cols:
            self.status[i] = STATUS_KKT_LIMIT

    def _finish(self, idx, status):
        for i in idx:
            self.status[i] = status
        self.live[idx] = False

    def step(self, time_left: bool = True):
        """one segment: iterations up to the next check (or the first LP's KKT-pass cap), then the check and the restarts"""
        live = self.live.copy()
        if not self._segment(live, time_left):
            return
        if self.k_global % self.period == 0:                                 # pdhg.py:115 (tt = k mod period for every live LP)
            action, capped, chosen = self._halpern_check(live) if self.halpern else self._restart_check(live)
        else:                                                                # only the cap ends an inner loop between checks
            capped = live & (self.j >= self.max_kkt)
            action, chosen = np.where(capped, 1, 0).astype(np.int32), None
        if self.halpern:           # a capped LP keeps its candidate (inside the bounds), never the reflected iterate
            action = np.where(capped & (self.tt > 0), 2, action).astype(np.int32)
        if action.any():
            self._after_restart(action, capped, chosen)

    def _segment(self, live, time_left: bool) -> bool:
        """PDHG iterations of every live LP up to the next check or the first KKT-pass cap (pdhg.py:76-112); False when the clock
        or the cap ends the batch instead"""
        if not time_left:                                                    # pdhg.py:68-74, the global clock
            if self.halpern and (live & (self.tt > 0)).any():                # the returned point is the candidate, as in run_pdlp
                self.be.set_scalars(action=np.where(live & (self.tt > 0), 2, 0).astype(np.int32))
                self.be.restart(0)
                self.be.set_scalars(action=np.zeros(self.be.B, np.int32))
            self._finish(np.flatnonzero(live), STATUS_TIME_LIMIT)
            return False
        iters = min(self.period - self.k_global % self.period, int((self.max_kkt - self.j[live]).min()))
        if iters <= 0:                                                       # max_kkt <= 0: the reference's loop never runs
            self._finish(np.flatnonzero(live), STATUS_KKT_LIMIT)
            return False
        if self.halpern:
            self.be.halpern_iterate(iters, self.tt)
        else:
            self.be.iterate(iters, self.adaptive, self.k_global)
        self.k_global += iters
        self.k[live] += iters
        self.j[live] += iters
        self.tt[live] += iters
        return True

    def _restart_check(self, live):
        """pdhg.py:115-146 for every live LP: three KKT passes, one host read -> (action, capped, the residuals at the chosen iterate)"""
        be, t = self.be, self.t
        be.average(self.adaptive)                                            # pdhg.py:118-119
        for slot, which in enumerate((N.CUR, N.AVG, N.PREV)):               # pdhg.py:122-125
            be.kkt(which, slot)
        out = be.read_out()
        r = [kkt_from_sums(out[s], self.omega, t) for s in range(3)]
        self.j[live] += 3                                                    # pdhg.py:128
        dec = restart_decision(r[0]["kkt"], r[1]["kkt"], r[2]["kkt"], self.kkt_first, self.tt, self.k, self.j, live, self.max_kkt, t)
        if self.traces is not None:
            for i in np.flatnonzero(live):
                tr = self.traces[self.lp[i]]
                tr["kkt"] += [float(r[0]["kkt"][i]), float(r[1]["kkt"][i]), float(r[2]["kkt"][i])]
                if dec["crit"][i] >= 0:
                    tr["restarts"].append((int(dec["crit"][i]), int(self.tt[i]), int(dec["use_avg"][i])))
        chosen = {key: np.where(dec["use_avg"], r[1][key], r[0][key]) for key in r[0]}
        return dec["action"], dec["capped"], chosen

    def _halpern_check(self, live):
        """the restart check of the Halpern mode for every live LP: one KKT pass at the candidate, one host read, the rules of
        ``restart_decision`` unchanged -> (action, capped, the residuals at the candidate)"""
        be, t = self.be, self.t
        be.kkt(N.AVG, 1)
        r = kkt_from_sums(be.read_out()[1], self.omega, t)
        self.j[live] += 1
        k_cur, k_cand, k_prev = np.full(be.B, np.inf, t), t(r["kkt"]), self.k_prev_cand.copy()
        self.k_prev_cand[live] = k_cand[live]
        dec = restart_decision(k_cur, k_cand, k_prev, self.kkt_first, self.tt, self.k, self.j, live, self.max_kkt, t)
        if self.traces is not None:
            for i in np.flatnonzero(live):
                tr = self.traces[self.lp[i]]
                tr["kkt"] += [float(k_cur[i]), float(k_cand[i]), float(k_prev[i])]
                if dec["crit"][i] >= 0:
                    tr["restarts"].append((int(dec["crit"][i]), int(self.tt[i]), 1))
        action = np.where(dec["crit"] >= 0, 2, dec["action"]).astype(np.int32)       # a restart is always at the candidate
        return action, dec["capped"], r

    def _after_restart(self, action, capped, chosen):
        """pdhg.py:148-177 for the LPs that leave their inner loop: n += 1, primal weight, KKT_first, residuals, termination test"""
        be, t = self.be, self.t
        act = np.flatnonzero(action)
        be.set_scalars(action=action)
        be.restart(0)
        if capped.any():           # no check chose their point: a pass at the current iterate (pdhg.py:153 after the cap)
            be.kkt(N.CUR, 2)
        if self.precondition:
            be.kkt(N.CUR, 1, unscaled=True)                                  # pdhg.py:157-163
        out = be.read_out()
        be.set_scalars(action=np.zeros(be.B, np.int32))
        self.n[act] += 1
        self.tt[act] = 0
        self.k_prev_cand[act] = np.inf
        if self.primal_update:                                               # pdhg.py:150-151
            self.omega[act] = primal_weight(out[0, act, 0], out[0, act, 1], self.omega[act], 0.5, t)
            be.set_scalars(omega=self.omega)
            if self.traces is not None:
                for i in act:
                    self.traces[self.lp[i]]["omega"].append(float(self.omega[i]))
        if capped.any():
            rc = kkt_from_sums(out[2], self.omega, t)
            chosen = rc if chosen is None else {key: np.where(capped, rc[key], chosen[key]) for key in rc}
        kf = kkt_error(chosen, self.omega, t)                                # pdhg.py:153-154
        self.kkt_first[act] = kf[act]
        self.j[act] += 2                                                     # pdhg.py:154,165
        if self.traces is not None:
            for i in act:
                self.traces[self.lp[i]]["kkt"].append(float(kf[i]))
        res = kkt_from_sums(out[1], self.omega, t) if self.precondition else chosen
        self.obj[act] = res["p"][act].astype(np.float64)
        solved = terminated(res, self.q_norm, self.c_norm, self.tol, t)      # pdhg.py:173
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


def start_scalars(sigma, q_norm, c_norm, t):
    """pdhg.py:22-23 per LP: the start ``(eta, omega)`` [B] from sigma (one for the batch, or [B]) and the norms [B]"""
    omega = start_omega(q_norm, c_norm, t)
    return np.broadcast_to(np.asarray(start_eta(np.asarray(sigma, t), t), t), np.shape(omega)), omega


def estimate_sigma_batch(be: BatchEngine, b0=None, power_iters=100, seed=None) -> np.ndarray:
    """``estimate_sigma`` per LP of a batch with a matrix each: the reference's power iteration column by column on the population
    product, from the same start vector (``b0``, or drawn from ``seed`` as ``estimate_sigma`` draws it) for every LP"""
    if b0 is None:
        b0 = power_iteration_start(be.n, seed)
    return be.power_iteration(b0.to(be.device), power_iters)


def check_slots(slots, B: int, W, dtype, per_lp_matrices: bool, precondition: bool) -> bool:
    """whether ``slots`` asks for a streamed solve of ``B`` LPs (None, or at least B: the plain batch); ValueError for a width the
    launches cannot have or a combination that has no streamed form -- before any device work"""
    if slots is None:
        return False
    if isinstance(slots, bool) or int(slots) != slots or slots < 1:
        raise ValueError(f"slots must be a positive number of columns, got {slots!r}")
    if slots >= B:
        return False
    W = int(W) if W is not None else group_width(int(slots), dtype)
    if W not in (8, 16, 32) or slots % W != 0:
        raise ValueError(f"slots must be a multiple of the group width {W} (8, 16 or 32: group_width), got {slots}")
    if per_lp_matrices and precondition:
        raise ValueError("K_values with precondition has no streamed form (a Ruiz equilibration per LP in chunks): solve it with "
                         "slots=None, or equilibrate the matrices beforehand")
    return True


def _column_norms(v: torch.Tensor, B: int, t, device, chunk: Optional[int]) -> np.ndarray:
    """pdhg.py:19-20 per LP (as solver._global_norm: the float64 norm of every column, rounded to the working precision), computed
    where ``v`` is; with ``chunk``, an array that stays on the host goes to the device that many columns at a time"""
    v = v.reshape(v.shape[0], -1)
    norm = lambda w: np.sqrt((w.double() ** 2).sum(0).cpu().numpy())
    if chunk is None or v.device == device or v.shape[1] == 1:
        return np.broadcast_to(norm(v), (B,)).astype(t)
    return np.concatenate([norm(v[:, a:a + chunk].to(device)) for a in range(0, B, chunk)]).astype(t)


def _setup(be: BatchEngine, B: int, Q, C_, K_values, perm, b0, sigma, seed, setup_times):
    """pdhg.py:19-22 for the B LPs of a solve over ``be``: ``(q_norm, c_norm, sigma)``.  sigma when not given: once for a shared K,
    per LP for a matrix each -- of a family longer than ``be`` is wide in chunks of its columns, each chunk's values through the
    attached populations (the admissions overwrite them)."""
    t, chunk = np_type(be.dtype), be.B if be.B < B else None
    qn, cn = _column_norms(Q, B, t, be.device, chunk), _column_norms(C_, B, t, be.device, chunk)
    if sigma is None:
        ts = time.time()
        if K_values is None:
            sigma = estimate_sigma(be.eng, b0, 100, seed)
        elif chunk is None:
            sigma = estimate_sigma_batch(be, b0, 100, seed)
        else:
            b0, parts = power_iteration_start(be.n, seed) if b0 is None else b0, []
            for a in range(0, B, chunk):
                cnt = min(chunk, B - a)
                with torch.cuda.stream(be.stream):
                    be.K_valB[:, :cnt] = K_values[:, a:a + cnt].to(device=be.device, dtype=be.dtype)
                    be.KT_valB.copy_(be.K_valB[perm])
                parts.append(estimate_sigma_batch(be, b0, 100)[:cnt])
            sigma = np.concatenate(parts)
        if setup_times is not None:
            setup_times["power_iteration_seconds"] = time.time() - ts
    return qn, cn, sigma


def _fill_report(report, be: BatchEngine, precondition, Y, rc, act, qn, cn, sums, omega):
    """the solution report of the returned iterates (``Y`` scaled, as the batch holds it) into the caller's dict"""
    if report is not None:
        report.update(y=Y * be.d_row if precondition else Y.clone(), reduced_costs=rc, row_activity=act, q_norm=qn, c_norm=cn,
                      **kkt_from_sums(sums, omega, np_type(be.dtype)))


def _solve_stream(drv: BatchDriver, B, perm, C_, Q, L, U, x_init, y_init, K_values, qn, cn, sigma, time_left, verbose, want_report,
                  schedule):
    """``pdlp_algorithm_batch`` for a family longer than the batch is wide: the columns of ``drv.be``, the LPs queued in index order.

    After every restart check of the batch (``k_global`` a multiple of the period) the columns whose LP has finished are retired
    (``pdlp_batch_retire``: iterate and report into the LP's column of the results) and given to the next LPs
    (``pdlp_batch_admit``).  ``StreamQueue`` (rules.py) says why an admitted LP runs the control flow of a batch that started with
    it; the adaptive rule counts from its admission (``k_start``), and no kernel makes an LP's bits depend on its column: the
    results are those of the plain batch at the same W.  Per check still one host read; the sums of the retirements are fetched
    once, at the end.  Device memory: the state of ``slots`` LPs, the ``(n + m, B)`` results, and one admission's columns.
    Returns ``(X, Y, rc, act, sums, res)``: the results [len, B] (rc, act None unless ``want_report``), the six sums [B, 6] and the
    per-LP counters, objective, primal weight and status."""
    be, t = drv.be, drv.t
    dev, dt, slots = be.device, be.dtype, be.B
    be.enable_stream()
    eta0, omega0 = start_scalars(sigma, qn, cn, t)
    drv.live[:] = False
    queue = StreamQueue(B, slots, drv.period)
    X = torch.zeros(be.n, B, dtype=dt, device=dev)
    Y = torch.zeros(be.m, B, dtype=dt, device=dev)
    rc, act = (torch.zeros(be.n, B, dtype=dt, device=dev), torch.zeros(be.m, B, dtype=dt, device=dev)) if want_report else (None, None)
    sums = torch.zeros(B, 6, dtype=torch.float64, device=dev)
    res = dict(k=np.zeros(B, np.int64), n=np.zeros(B, np.int64), j=np.zeros(B, np.int64), obj=np.full(B, np.nan),
               omega=np.array(omega0, t), status=[STATUS_TIME_LIMIT] * B)

    def stage(v, a, b, shared_ok=True):
        """columns [a, b) of a source array as a feed array: [len, b - a] on the device (None: shared by the batch / zeros)"""
        if v is None or (shared_ok and (v.dim() == 1 or v.shape[1] == 1)):
            return None
        if v.dim() == 1 or v.shape[1] == 1:                                  # one start point for every LP
            return v.reshape(-1, 1).to(device=dev, dtype=dt).expand(-1, b - a).contiguous()
        return v[:, a:b].to(device=dev, dtype=dt).contiguous()

    def admit_cols(cols, ids):
        a, b = int(ids[0]), int(ids[-1]) + 1                                 # (the queue hands the LPs out in index order)
        with torch.cuda.stream(be.stream):
            Kv = stage(K_values, a, b, shared_ok=False)
            be.admit(cols, np.arange(b - a), eta0[a:b], omega0[a:b], stage(C_, a, b), stage(Q, a, b), stage(L, a, b), stage(U, a, b),
                     stage(x_init, a, b, shared_ok=False), stage(y_init, a, b, shared_ok=False), Kv, None if Kv is None else Kv[perm])
        return slice(a, b)

    def retire_cols(cols, ids):
        be.retire(cols, ids, X, Y, rc, act, N.CUR, unscaled=drv.precondition)
        with torch.cuda.stream(be.stream):
            sums[torch.from_numpy(ids).to(dev)] = be.retire_out[0][torch.from_numpy(cols).to(dev)]

    def admit():
        cols, ids = queue.admit(drv.k_global)
        if not cols.size:
            return
        lps = admit_cols(cols, ids)
        drv.occupy(cols, ids, qn[lps], cn[lps], omega0[lps])
        ks = np.zeros(slots, np.int64)
        ks[queue.occupied()] = queue.admitted_at[queue.lp[queue.occupied()]]
        be.set_scalars(k_start=ks, live=drv.live.astype(np.int32))

    def retire(cols):
        if not cols.size:
            return
        ids = queue.retire(cols, drv.k_global)
        retire_cols(cols, ids)
        for key, arr in (("k", drv.k), ("n", drv.n), ("j", drv.j), ("obj", drv.obj), ("omega", drv.omega)):
            res[key][ids] = arr[cols]
        for c_, i in zip(cols, ids):
            res["status"][i] = drv.status[c_]

    admit()
    in_time = True
    while queue.occupied().size:
        if drv.live.any():
            in_time = time_left()
            drv.step(in_time)
        if not drv.live.any():               # nothing runs: the clock of the batch may move to its next check
            drv.k_global = queue.next_boundary(drv.k_global)
        if queue.may_admit(drv.k_global):
            occ = queue.occupied()
            retire(occ[~drv.live[occ]])
            if in_time:
                admit()
        if verbose:
            print(f"[batch] k={drv.k_global} live={int(drv.live.sum())}/{slots} waiting={queue.waiting()}")
    late = queue.never_admitted()            # the clock ran out before their turn: k = 0, the start point, its report
    sched = queue.schedule()
    while queue.waiting():
        cols, ids = queue.admit(queue.next_boundary(drv.k_global))
        admit_cols(cols, ids)
        queue.retire(cols, drv.k_global)
        retire_cols(cols, ids)
    if schedule is not None:
        schedule.update(sched, slots=slots, group_width=be.W, never_admitted=late)
    return X, Y, rc, act, sums, res


def pdlp_algorithm_batch(K, m_ineq, C_, Q, L, U, device=None, max_kkt=100_000, tol=1e-4, verbose=False, restart_period=40,
                         precondition=False, primal_update=False, adaptive=False, data_precond=None, time_limit=3600, time_used=0,
                         x_init=None, y_init=None, *, b0=None, sigma=None, seed=None, traces=None, group_width=None,
                         report=None, K_values=None, KT_values=None, setup_times=None, slots=None, schedule=None,
                         halpern=False):
    """``pdlp_algorithm`` on B LPs with the same ``K`` at once.  ``C_``, ``Q``, ``L``, ``U``: 1-D (shared) or [len, B] (one column
    per LP), of the scaled problem when ``precondition`` (then ``data_precond`` = ``ruiz_precondition``'s: ``D_col``, ``D_row``
    give the un-scaled residuals).  ``traces``: a list of B dicts (``kkt``, ``omega``, ``restarts``) that receive every LP's trace.
    ``group_width``: W (8, 16, 32; default by B and dtype) -- results are bit-identical across batches of the same W.
    ``report``: a dict that receives the solution report of the returned iterates -- ``y`` [m, B], ``reduced_costs`` [n, B],
    ``row_activity`` [m, B] and [B] arrays ``pr, dr, gap, p, d_adj, kkt`` (helpers.py:53-108), of the ORIGINAL problems when
    ``precondition`` -- whatever each LP's status; ``q_norm``, ``c_norm`` [B]: the norms the termination test used.
    ``K_values`` ``(nnz, B)``: a matrix per LP over K's pattern, column b the values of LP b in the order of ``K.val``
    (``KT_values``: the same values in the order of ``K.t_val``; permuted here when omitted).  Then ``data_precond`` is
    ``(D_col (n, B), D_row (m, B))``, every LP's own Ruiz factors (``ruiz_precondition_batch``), the step size comes from a power
    iteration per LP, and ``sigma`` may be one number or a [B] array.  ``setup_times``: a dict that receives
    ``power_iteration_seconds`` when sigma is estimated here.
    ``slots`` < B: the family is streamed through ``slots`` columns (``_solve_stream``: the same results, bit for bit, from the
    memory of ``slots`` LPs); ``c, q, l, u, x_init, y_init, K_values`` may then stay on the host.  ``schedule``: a dict that receives
    ``column``, ``admitted_at``, ``retired_at`` ([B]) of such a run.
    ``halpern`` (the reference has no counterpart): the restarted, reflected Halpern iteration per LP instead of averaged PDHG, with
    the fixed step (``BatchDriver``); every returned iterate is a candidate, inside the bounds.  ``ValueError`` with
    ``adaptive``.
    Returns ``(X, Y, obj, k, n, j, status, total_time)`` with X [n, B], Y [m, B] (the scaled iterates when preconditioned, like
    ``pdlp_algorithm``'s x) and numpy arrays / a list of status strings per LP."""
    t0 = time.time()
    if halpern and adaptive:
        raise ValueError(HALPERN_BATCH_REFUSED)
    B = batch_size(C_, Q, L, U, K_values)
    streamed = check_slots(slots, B, group_width, K.val.dtype if isinstance(K, CsrPair) else C_.dtype, K_values is not None, precondition)
    Kp = CsrPair.from_any(K, device=resolve_device(device))
    if K_values is not None and tuple(K_values.shape) != (Kp.nnz, B):
        raise ValueError(f"K_values must have shape ({Kp.nnz}, {B}), got {tuple(K_values.shape)}")
    for name, v, ln in (("x_init", x_init, Kp.n), ("y_init", y_init, Kp.m)):
        if v is not None and (v.dim() not in (1, 2) or v.shape[0] != ln or (v.dim() == 2 and v.shape[1] != B)):
            raise ValueError(f"{name} must have shape ({ln},) or ({ln}, {B}), got {tuple(v.shape)}")
    d_col, d_row = precond_factors(precondition, data_precond)
    if streamed and KT_values is not None:
        raise ValueError("a streamed family takes K_values only (the values of K' are permuted per admission)")
    dev, dt = Kp.val.device, Kp.val.dtype
    width = int(slots) if streamed else B            # the columns of the batch; a streamed family's first LPs start in them
    head = lambda v: v if not streamed else (v[:, :width] if v.dim() == 2 and v.shape[1] > 1 else v.reshape(-1)).to(device=dev, dtype=dt)
    be = BatchEngine(Kp, m_ineq, head(C_), head(Q), head(L), head(U), width, d_col=d_col, d_row=d_row, W=group_width,
                     K_values=None if K_values is None else K_values[:, :width], KT_values=KT_values)
    perm = Kp.transpose_perm() if streamed and K_values is not None else None
    qn, cn, sigma = _setup(be, B, Q, C_, K_values, perm, b0, sigma, seed, setup_times)
    drv = BatchDriver(be, qn[:width].copy(), cn[:width].copy(), restart_period, primal_update=primal_update, adaptive=adaptive,
                      precondition=precondition, tol=tol, max_kkt=max_kkt, traces=traces, halpern=halpern)
    time_left = lambda: time.time() - t0 + time_used < time_limit
    if streamed:
        X, Y, rc, act, sums, res = _solve_stream(drv, B, perm, C_, Q, L, U, x_init, y_init, K_values, qn, cn, sigma, time_left, verbose,
                                                 report is not None, schedule)
        _fill_report(report, be, precondition, Y, rc, act, qn, cn, sums.cpu().numpy(), res["omega"])
        be.synchronize()
        return X, Y, res["obj"], res["k"], res["n"], res["j"], res["status"], time.time() - t0 + time_used
    drv.start(sigma, x_init, y_init)
    while drv.live.any():
        drv.step(time_left())
        if verbose:
            print(f"[batch] k={drv.k_global} live={int(drv.live.sum())}/{B}")
    if report is not None:
        rc, act, sums = be.report(N.CUR, unscaled=bool(precondition))
        _fill_report(report, be, precondition, be.y[:, :B], rc.clone(), act.clone(), qn, cn, sums, drv.omega)
    be.synchronize()
    return (be.x[:, :B].clone(), be.y[:, :B].clone(), drv.obj, drv.k, drv.n, drv.j, list(drv.status), time.time() - t0 + time_used)
