"""Restarted PDHG outer loop on top of the HIP engine -- the drop-in for the reference's
``pdlp_algorithm`` (``/root/reference/PDLP/primal_dual_hybrid_gradient.py:7-181``).

Same arguments, same result tuple ``(x, prim_obj, k, n, j, status, total_time)``, same status
strings and the same KKT-pass bookkeeping ``j``.  The host only decides restarts: it reads three
KKT errors every ``restart_period`` iterations; everything else stays on the device.
"""
from __future__ import annotations

import time
from typing import Optional

import numpy as np
import torch

from . import _native as N
from .engine import Comm, PdlpEngine
from .rules import (STATUS_KKT_LIMIT, STATUS_SOLVED, STATUS_TIME_LIMIT, fixed_point_error, fixed_point_restart_decision,   # noqa: F401
                    kkt_error, np_type, previous_kkt_matters, primal_weight, qp_eta, restart_decision, start_eta, start_omega, terminated)
from .compose import HALPERN_REFUSED, check_composition, check_quad_step     # noqa: F401  (HALPERN_REFUSED: importable from here)
from .quad import check_quad_diag, check_quad_matrix
from .ranged import check_row_upper, norm_vector as ranged_norm_vector
from .sparse import CsrPair, as_vec, resolve_device     # noqa: F401  (resolve_device: api.py and callers take it from here)


def check_termination(primal_residual, dual_residual, duality_gap, prim_obj, adjusted_dual, q_norm, c_norm, tol):
    """check_termination with the reference's signature (helpers.py:110-128): ``rules.terminated`` on the values as they come"""
    res = dict(pr=primal_residual, dr=dual_residual, gap=duality_gap, p=prim_obj, d_adj=adjusted_dual)
    return bool(terminated(res, q_norm, c_norm, tol, t=lambda v: v))


kkt_from_residuals = kkt_error
HALPERN_RESTARTS = ("kkt", "fixed_point")
primal_weight_from_distances = primal_weight


def check_halpern_restart(halpern_restart, halpern) -> str:
    """``halpern_restart`` as given to a solve: one of ``HALPERN_RESTARTS``, and anything but "kkt" only with ``halpern=True``
    (``ValueError`` otherwise: the callers check before any device work)"""
    if halpern_restart not in HALPERN_RESTARTS:
        raise ValueError(f"unknown halpern_restart {halpern_restart!r}: one of {', '.join(map(repr, HALPERN_RESTARTS))}")
    if halpern_restart != "kkt" and not halpern:
        raise ValueError(f"halpern_restart={halpern_restart!r} is a restart rule of the Halpern mode: it needs halpern=True")
    return halpern_restart


def precond_factors(precondition, data_precond):
    """``(D_col, D_row)`` of ``ruiz_precondition``'s ``data_precond`` when ``precondition``, else ``(None, None)``"""
    if not precondition:
        return None, None
    if data_precond is None:
        raise ValueError("precondition=True needs data_precond from ruiz_precondition")
    return data_precond[0], data_precond[1]


def is_mixed(precision) -> bool:
    """whether ``precision`` asks for float32 matrix entries under float64 vectors; anything but None / "mixed" is an error"""
    if precision not in (None, "mixed"):
        raise ValueError(f"unknown precision {precision!r}")
    return precision == "mixed"


def _global_norm(v_local: torch.Tensor, comm: Optional[Comm]) -> float:
    s = (v_local.double() ** 2).sum().reshape(1)
    if comm is not None:
        comm.all_reduce_sum(s)
    return float(torch.sqrt(s))


class PdhgDriver:
    """The reference's two nested loops (pdhg.py:54-177) as a resumable state machine over an engine.

    ``advance(max_iters)`` runs PDHG iterations up to the next restart check (every
    ``restart_period`` iterations since the last restart), performs the check, and on a restart does the
    post-restart work (primal weight, KKT_first, termination test).  ``run_pdlp`` loops over it; the
    benchmark times the very same calls.

    ``halpern=True``: the restarted, reflected Halpern iteration (rHPDHG) instead of averaged PDHG, with the fixed step.  A segment
    is ``eng.halpern_iterate``; a check evaluates ONE point, the candidate ``N.AVG`` (one PDHG step from the Halpern iterate: inside
    the bounds), and hands ``restart_decision`` ``kkt_cur = inf``, ``kkt_avg`` = the candidate's KKT error and ``kkt_prev`` = the
    candidate's error at the previous check of this restart period (``inf`` at the first) -- so the decision is "restart at the
    candidate" or "keep"; ``after_restart`` runs as it is.  KKT-pass accounting: ``j += iters`` per segment, ``j += 1`` per check,
    and the two of ``after_restart``.

    ``halpern_restart="fixed_point"`` (with ``halpern``; default "kkt" = the paragraph above): the restart decision looks at the
    fixed-point residual ``r = ||z - T(z)||_P`` of the last iteration instead (``eng.halpern_fixed_point``, one product and no KKT
    pass; ``rules.fixed_point_error`` / ``fixed_point_restart_decision``).  ``r0``, the residual at the restart point, is evaluated
    after the first iteration of every restart period -- a segment that starts a period is ``halpern_iterate(1)``, the evaluation,
    ``halpern_iterate(rest)``; the checks stay on the multiples of the period.  ``j += 1`` per evaluation, ``r0`` included.
    ``after_restart`` runs as it is: it adopts the candidate, and its KKT pass at the restart point is the termination test.

    A sparse quadratic objective (the engine's ``quad_matrix``): the engine takes the linearised step, whose fixed step size
    ``rules.qp_eta(sigma, quad_norm, omega)`` depends on the primal weight -- ``start`` takes ``quad_norm`` (the estimate of ``||Q||_2``)
    and ``after_restart`` sets the step anew (``eng.set_step``) where it would set the primal weight alone (``eng.set_omega``).  A
    ``trace`` receives every step size set under ``"eta"``.  Averaged PDHG only; ``adaptive`` stays refused.
    ``quad_step="adaptive"`` (default "fixed" = the sentences above): a segment is ``eng.objective_iterate`` -- the linearised step
    under the step-size rule whose denominator carries the measured curvature ``dx'Q dx`` (include/pdlp_hip.h,
    pdlp_objective_iterate).  The start step is ``rules.qp_eta`` as before; from there the rule owns the step size,
    so a restart that changes the primal weight sets the weight alone (``eng.set_omega``) and the average is flushed as for an
    adaptive LP solve, whose KKT-pass accounting this mode has.  ``ValueError`` without a ``quad_matrix`` engine.
    """

    def __init__(self, eng: PdlpEngine, restart_period=40, primal_update=False, adaptive=False, precondition=False,
                 tol=1e-4, verbose=False, trace=None, infeasibility_detect=False, infeas_tol=1e-4, adaptive_retry=False,
                 halpern=False, halpern_restart="kkt", quad_step="fixed"):
        self.eng, self.period = eng, int(restart_period)
        self.halpern = bool(halpern)
        self.fixed_point = check_halpern_restart(halpern_restart, self.halpern) == "fixed_point"
        self.eta = None                                                     # the fixed step of the run (start)
        self.r0 = self.r_prev = None                                        # fixed-point rule: the residual at the restart point / at the previous check
        form = dict(adaptive_retry=adaptive_retry, infeasibility_detect=infeasibility_detect, mixed=getattr(eng, "mixed", False), comm=eng.comm is not None)
        check_composition(halpern=self.halpern, adaptive=adaptive, **form)
        q_upper = getattr(eng, "q_upper", None)     # (a refusal comes before anything more of the engine is read: one switch at a time)
        check_composition(q_upper=q_upper is not None, **form)
        check_composition(quad_diag=getattr(eng, "quad_diag", None) is not None, **form)
        self.quad = getattr(eng, "quad_matrix", None) is not None
        check_composition(quad_matrix=self.quad, halpern=self.halpern, adaptive=adaptive, **form)
        self.quad_adaptive = check_quad_step(quad_step, self.quad) == "adaptive"     # (the rule owns eta: objective_iterate)
        self.sigma = self.quad_norm = None                                  # the norm estimates the step rule of quad_matrix keeps
        self.kkt_prev_cand = None                                           # Halpern: the candidate's KKT error at the previous check
        self.infeasibility_detect, self.infeas_tol = bool(infeasibility_detect), float(infeas_tol)
        self.infeasible = None                                              # the detector's verdict (pdhg.py:94-100)
        # SURVEY quirk Q1's optional flag: the adaptive step as it was meant (enhancements/test_ass.py:322-363) -- a rejected trial is
        # discarded and repeated with the shrunk step size until one is accepted (at most 200, like the reference's loop bound);
        # one KKT-pass count per trial (step.py:93 sits inside the loop).  Off: the live package's single trial (a rejected step is kept)
        self.adaptive_retry = bool(adaptive_retry) and bool(adaptive)
        self.trials = 0
        self.primal_update, self.adaptive, self.precondition = bool(primal_update), bool(adaptive), bool(precondition)
        self.tol, self.verbose, self.trace = tol, verbose, trace
        self.t = np_type(eng.dtype)
        # pdhg.py:19-20; with two-sided rows (the engine's q_upper) ||q|| is the norm of max(|q_i|, |q_upper_i|) on those rows
        self.q_norm = self.t(_global_norm(ranged_norm_vector(eng.q, q_upper, getattr(eng, "m_ineq", 0)), eng.comm))
        self.c_norm = self.t(_global_norm(eng.c, eng.comm))
        self.n = self.k = self.j = self.tt = 0
        self.KKT_first = self.t(0)                                          # pdhg.py:48
        self.omega = self.t(1)
        self.res = None
        self.solved = False
        self.checks = 0                # restart checks performed (pdhg.py:115)
        self.check_seconds = None      # set to 0.0 to accumulate the wall time of the restart checks (synchronises around them)

    def _set_quad_step(self, k=0):
        """quad_matrix: the step that goes with the current primal weight, to the engine (and the trace)"""
        self.eta = qp_eta(self.sigma, self.quad_norm, self.omega, self.t)
        self.eng.set_step(self.eta, self.omega, 1.0, k)
        if self.trace is not None:
            self.trace.setdefault("eta", []).append(float(self.eta))

    def start(self, sigma, x_init=None, y_init=None, theta=1.0, quad_norm=0.0):
        t, eng = self.t, self.eng
        self.omega = start_omega(self.q_norm, self.c_norm, t)               # pdhg.py:23
        self.sigma, self.quad_norm = float(sigma), float(quad_norm)
        eta = qp_eta(sigma, quad_norm, self.omega, t) if self.quad else start_eta(sigma, t)      # pdhg.py:22
        zeros = lambda ln: torch.zeros(ln, dtype=eng.dtype, device=eng.device)
        if x_init is not None and y_init is not None:                       # pdhg.py:31-36
            eng.set_iterate(x_init, y_init)
        else:
            eng.set_iterate(zeros(eng.nl), zeros(eng.ml))
        eng.set_step(eta, self.omega, theta, 0)
        self.eta = eta
        if self.quad and self.trace is not None:
            self.trace.setdefault("eta", []).append(float(eta))
        self.r0 = self.r_prev = None
        if self.infeasibility_detect:
            eng.infeas_reset()                                              # pdhg.py:39-40
        self.n = self.k = self.j = self.tt = 0
        self.KKT_first = t(0)
        self.res, self.solved, self.infeasible = None, False, None
        self.kkt_prev_cand = None

    def advance(self, max_iters: int) -> int:
        """Iterate up to the next restart check (at most ``max_iters``); returns the iterations done."""
        iters, at_check = self._segment(int(max_iters))
        if at_check:
            self._restart_check()
        return iters

    def _segment(self, max_iters: int):
        """PDHG iterations up to the next check, ``max_iters`` at most (pdhg.py:76-112) -> (iterations done, whether a check is due)"""
        eng = self.eng
        if self.infeasibility_detect:
            # the detector looks at every iterate (pdhg.py:89-101): one iteration per call, one more pass each (max_iters bounds the passes)
            iters, j0 = 0, self.j
            while True:
                eng.iterate(1, self.adaptive)
                self.k += 1
                self.j += 1
                iters += 1
                if self.k > 1:                                              # "need at least two points"
                    self.infeasible = eng.detect_infeasibility(self.infeas_tol)
                    self.j += 1                                             # pdhg.py:93
                    if self.infeasible:
                        if self.verbose:
                            print(f"[PDLP] {self.infeasible} detected at iteration {self.k}")
                        return iters, False
                self.tt += 1
                if self.tt % self.period == 0:
                    return iters, True
                if self.j - j0 >= max_iters:                                # pdhg.py:67
                    return iters, False
        iters = min(self.period - self.tt % self.period, max_iters)
        if iters <= 0:
            return 0, False
        if self.halpern and self.fixed_point and self.tt == 0:
            # the first iteration of a restart period starts at the anchor: its residual is r0 (with the omega of this period)
            eng.halpern_iterate(1)
            self.r0, self.r_prev = fixed_point_error(*eng.halpern_fixed_point(), self.eta, self.omega), None
            self.j += iters + 1
            if iters > 1:
                eng.halpern_iterate(iters - 1)
        elif self.halpern:
            eng.halpern_iterate(iters)
            self.j += iters
        elif self.adaptive_retry:                    # every iteration is tried until a step is accepted, one KKT-pass count per trial
            for _ in range(iters):
                trials = 0
                while True:
                    eng.iterate(1, True)
                    trials += 1
                    if trials >= 200 or eng.scalars()["accepted"]:         # (one host read per trial: this mode is not the fast path)
                        break
                    eng.adaptive_retry()
                self.j += trials
                self.trials += trials
        elif self.quad_adaptive:
            eng.objective_iterate(iters)
            self.j += iters
        else:
            eng.iterate(iters, self.adaptive)
            self.j += iters
        self.k += iters
        self.tt += iters
        return iters, self.tt % self.period == 0                            # pdhg.py:115

    def _halpern_check(self):
        """the restart check of the Halpern mode: one KKT pass at the candidate, the rules of ``restart_decision`` unchanged"""
        eng, t = self.eng, self.t
        timed = self.check_seconds is not None
        if timed:
            eng.synchronize()
            t_check = time.perf_counter()
        self.checks += 1
        with N.trace_range("pdlp: restart check (Halpern candidate)", getattr(eng, "stream", None)):
            r_cand = eng.kkt(N.AVG, self.omega)
            k_cur, k_cand = t(np.inf), t(r_cand["kkt"])
            k_prev = t(np.inf) if self.kkt_prev_cand is None else self.kkt_prev_cand
            self.kkt_prev_cand = k_cand
            self.j += 1
            if self.trace is not None:
                self.trace["kkt"] += [float(k_cur), float(k_cand), float(k_prev)]
            dec = restart_decision(k_cur, k_cand, k_prev, self.KKT_first, self.tt, self.k, self.j, live=True, t=t)
        crit = int(dec["crit"])
        if crit >= 0:
            if self.verbose:
                print(f"{('Sufficient', 'Necessary', 'Artificial')[crit]} restart at iteration {self.tt} using the Halpern candidate.")
            if self.trace is not None:
                self.trace["restarts"].append((crit, self.tt, 1))
            with N.trace_range("pdlp: restart work (restart, primal weight, termination test)", getattr(eng, "stream", None)):
                eng.restart(N.AVG)
                self.kkt_prev_cand = None
                self.after_restart(r_cand)
        if timed:
            eng.synchronize()
            self.check_seconds += time.perf_counter() - t_check

    def _halpern_fixed_point_check(self):
        """the restart check under ``halpern_restart="fixed_point"``: one evaluation of the fixed-point residual, no KKT pass"""
        eng, t = self.eng, self.t
        timed = self.check_seconds is not None
        if timed:
            eng.synchronize()
            t_check = time.perf_counter()
        self.checks += 1
        with N.trace_range("pdlp: restart check (Halpern fixed-point residual)", getattr(eng, "stream", None)):
            r = fixed_point_error(*eng.halpern_fixed_point(), self.eta, self.omega)
            r_prev = np.inf if self.r_prev is None else self.r_prev
            self.r_prev = r
            self.j += 1
            if self.trace is not None:
                self.trace["kkt"] += [float(np.inf), float(r), float(r_prev)]
            dec = fixed_point_restart_decision(r, r_prev, self.r0, self.tt, self.k, self.j, live=True, t=t)
        crit = int(dec["crit"])
        if crit >= 0:
            if self.verbose:
                print(f"{('Sufficient', 'Necessary', 'Artificial')[crit]} restart at iteration {self.tt} using the Halpern candidate.")
            if self.trace is not None:
                self.trace["restarts"].append((crit, self.tt, 1))
            with N.trace_range("pdlp: restart work (restart, primal weight, termination test)", getattr(eng, "stream", None)):
                # no KKT pass was made at the candidate: after_restart adopts it (eng.restart(N.AVG), as it does when the KKT-pass cap
                # ends a period) and evaluates it as the new current iterate
                self.after_restart(None)
        if timed:
            eng.synchronize()
            self.check_seconds += time.perf_counter() - t_check

    def _restart_check(self):
        """pdhg.py:115-146: the three KKT errors, the decision and, when it says so, the restart with its work"""
        if self.halpern:
            return self._halpern_fixed_point_check() if self.fixed_point else self._halpern_check()
        eng, t = self.eng, self.t
        timed = self.check_seconds is not None
        if timed:
            eng.synchronize()
            t_check = time.perf_counter()
        self.checks += 1
        with N.trace_range("pdlp: restart check (3 KKT evaluations)", getattr(eng, "stream", None)):
            # the current iterate first: its pass keeps K'y, which closes the running sum of K'y_k -- the averaged iterate then
            # needs no product at all (K x_avg and K'y_avg come out of the sums; include/pdlp_hip.h, pdlp_flush_average)
            r_cur = eng.kkt(N.CUR, self.omega)                              # pdhg.py:122-125
            eng.flush_average(self.adaptive or self.quad_adaptive)
            eng.compute_average()                                           # pdhg.py:118-119
            r_avg = eng.kkt(N.AVG, self.omega)
            k_cur, k_avg = t(r_cur["kkt"]), t(r_avg["kkt"])
            # KKT_previous only enters the "necessary" test (pdhg.py:135); the reference evaluates it at every check.
            # Here it is evaluated when that test can fire (or when a trace is recorded); the decision and the pass
            # counter j are the same either way.
            need_prev = self.trace is not None or previous_kkt_matters(k_cur, k_avg, self.KKT_first, t)
            k_prev = t(eng.kkt(N.PREV, self.omega)["kkt"]) if need_prev else t(np.inf)
            self.j += 3                                                     # pdhg.py:128
            if self.trace is not None:
                self.trace["kkt"] += [float(k_cur), float(k_avg), float(k_prev)]
            dec = restart_decision(k_cur, k_avg, k_prev, self.KKT_first, self.tt, self.k, self.j, live=True, t=t)
        crit, use_avg = int(dec["crit"]), bool(dec["use_avg"])
        if crit >= 0:
            if self.verbose:
                print(f"{('Sufficient', 'Necessary', 'Artificial')[crit]} restart at iteration {self.tt} using the",
                      "Average iterate." if use_avg else "Current iterate.")
            if self.trace is not None:
                self.trace["restarts"].append((crit, self.tt, int(use_avg)))
            with N.trace_range("pdlp: restart work (restart, primal weight, termination test)", getattr(eng, "stream", None)):
                eng.restart(N.AVG if use_avg else N.CUR)
                self.after_restart(r_avg if use_avg else r_cur)
        if timed:
            eng.synchronize()
            self.check_seconds += time.perf_counter() - t_check

    def after_restart(self, chosen=None):
        """pdhg.py:148-177: n += 1, primal weight, KKT_first, residuals, termination test."""
        eng, t = self.eng, self.t
        self.n += 1
        since, self.tt = self.tt, 0
        if chosen is None and self.halpern and since > 0:
            # Halpern: the point that is inside the bounds is the candidate of the last iteration, not the reflected iterate
            eng.restart(N.AVG)
            self.kkt_prev_cand = None
        elif chosen is None:     # the KKT-pass cap ended the inner loop: continue from the current iterate
            eng.restart(N.CUR)
        if self.primal_update:                                              # pdhg.py:150-151
            dx2, dy2 = eng.restart_distance()
            omega_before = self.omega
            self.omega = primal_weight(dx2, dy2, self.omega, 0.5, t)
            if self.quad and not self.quad_adaptive and self.omega != omega_before:
                self._set_quad_step(self.k)          # (the step of the linearised iteration depends on the primal weight)
            else:
                eng.set_omega(self.omega)
            if self.trace is not None:
                self.trace["omega"].append(float(self.omega))
        eng.mark_restart_point()                                            # pdhg.py:63-64 of the next round
        if getattr(eng, "delta", False):
            # mixed precision, delta mode: the restart point's K x and K'y are recomputed exactly (float64 accumulation) -- this
            # bounds the drift of the running products and makes the termination test below an exact evaluation
            eng.refresh_products()
            chosen = eng.kkt(N.CUR, self.omega)
        if chosen is None:
            chosen = eng.kkt(N.CUR, self.omega)
        # KKT_first at the restart point with the (new) omega: the residuals do not depend on omega, so
        # the pass the reference repeats here (pdhg.py:153) is a re-weighting of numbers already known
        self.KKT_first = kkt_error(chosen, self.omega, t)
        self.j += 1                                                         # pdhg.py:154
        if self.trace is not None:
            self.trace["kkt"].append(float(self.KKT_first))
        res = eng.kkt(N.CUR, self.omega, unscaled=True) if self.precondition else chosen   # pdhg.py:157-163
        self.res = res
        self.j += 1                                                         # pdhg.py:165
        if self.verbose:
            print(f"[{self.k}] Primal Obj: {res['p']:.4f}, Adjusted Dual Obj: {res['d_adj']:.4f}, "
                  f"Gap: {res['gap'] / (1 + abs(res['p']) + abs(res['d_adj'])):.2e}, "
                  f"Prim Res: {res['pr'] / (1 + self.q_norm):.2e}, Dual Res: {res['dr'] / (1 + self.c_norm):.2e}\n")
        self.solved = bool(terminated(res, self.q_norm, self.c_norm, self.tol, t))


def power_iteration_start(n: int, seed=None) -> torch.Tensor:
    """the start vector of the power iteration, drawn on the host from ``seed`` (None: from the clock, as unpinned as the reference's)"""
    g = torch.Generator().manual_seed(int(seed) if seed is not None else int(time.time_ns() % (2 ** 31)))
    return torch.randn(n, generator=g, dtype=torch.float32)


def estimate_sigma(eng: PdlpEngine, b0=None, power_iters=100, seed=None) -> float:
    """spectral_norm_estimate_torch (helpers.py:41-51); the reference's start vector is an unseeded
    torch.randn (quirk Q6) -- here ``b0`` or ``seed`` pins it, and every rank uses the same vector."""
    if b0 is None:
        b0 = power_iteration_start(eng.n, seed).to(eng.device)
        if eng.comm is not None:
            eng.comm.dist.broadcast(b0, 0, group=eng.comm.group)
            part = getattr(eng, "part", None)
            if part is not None:                      # (drawn in the padded layout: padding variables have empty columns --
                keep = torch.zeros(eng.n, dtype=torch.bool, device=eng.device)       # zero their entries so that the start
                keep[part.col_map(eng.device)] = True                                # vector is one of the original LP)
                b0 = b0 * keep
    return eng.power_iteration(b0, power_iters)


def estimate_quad_norm(eng: PdlpEngine, b0=None, power_iters=100, seed=None) -> float:
    """The estimate of ``||Q||_2`` for ``rules.qp_eta``: ``estimate_sigma``'s recurrence (helpers.py:41-51) on the matrix of the
    engine's quadratic objective -- ``b <- Q'(Q b) / ||.||`` from the same start vector for the same number of iterations, then
    ``||Q b||`` -- through the plain product ``eng.objective_product``.  0 for a ``Q`` without stored entries."""
    if b0 is None:
        b0 = power_iteration_start(eng.n, seed)
    b = as_vec(b0, eng.n, eng.device, eng.dtype)
    for _ in range(int(power_iters)):
        b = eng.objective_product(eng.objective_product(b))
        nb = torch.linalg.norm(b)
        if float(nb) == 0.0:
            return 0.0
        b = b / nb
    return float(torch.linalg.norm(eng.objective_product(b)))


def run_pdlp(eng: PdlpEngine, max_kkt=100_000, tol=1e-4, verbose=True, restart_period=40, precondition=False,
             primal_update=False, adaptive=False, time_limit=3600, time_used=0, x_init=None, y_init=None,
             b0=None, sigma=None, power_iters=100, seed=None, trace=None, infeasibility_detect=False, infeas_tol=1e-4,
             adaptive_retry=False, *, report=None, halpern=False, halpern_restart="kkt", quad_norm=None, quad_step="fixed"):
    """The outer loop over an existing engine.  Returns (x_local, prim_obj, k, n, j, status, total_time).
    ``report``: a dict that receives ``PdlpEngine.report`` of the returned iterate (this rank's blocks; of the un-preconditioned
    problem when ``precondition``) whatever the status, and ``q_norm`` / ``c_norm`` as the termination test used them -- in the
    style of ``trace``.  ``halpern``: the restarted, reflected Halpern iteration (``PdhgDriver``); the returned iterate is then the
    candidate of the last restart or, when the run ends between restarts, of the last iteration.  ``halpern_restart``: "kkt" or
    "fixed_point", the quantity its restart checks look at (``PdhgDriver``).  ``quad_norm``: overrides the estimate of ``||Q||_2`` of an
    engine with a sparse quadratic objective (``estimate_quad_norm``), as ``sigma`` overrides that of ``||K||_2``.  ``quad_step``:
    "fixed" or "adaptive", the step rule of such an engine (``PdhgDriver``)."""
    t0 = time.time()
    check_halpern_restart(halpern_restart, halpern)
    if adaptive_retry and (getattr(eng, "delta", False) or infeasibility_detect):
        raise ValueError("adaptive_retry works on float32 / float64 engines without the infeasibility detector")
    drv = PdhgDriver(eng, restart_period, primal_update=primal_update, adaptive=adaptive, precondition=precondition, tol=tol,
                     verbose=verbose, trace=trace, infeasibility_detect=infeasibility_detect, infeas_tol=infeas_tol,
                     adaptive_retry=adaptive_retry, halpern=halpern, halpern_restart=halpern_restart, quad_step=quad_step)
    if sigma is None:                                                       # pdhg.py:22
        sigma = estimate_sigma(eng, b0, power_iters, seed)
    if drv.quad and quad_norm is None:
        quad_norm = estimate_quad_norm(eng, b0, power_iters, seed)
    drv.start(sigma, x_init, y_init, quad_norm=quad_norm if drv.quad else 0.0)
    status = STATUS_KKT_LIMIT
    while drv.j < max_kkt:                                                  # pdhg.py:54
        n_before = drv.n
        while drv.j < max_kkt and drv.n == n_before:                        # pdhg.py:67
            expired = time.time() - t0 + time_used >= time_limit            # pdhg.py:68-74
            # the reference looks at the clock before every iteration; here at least every ~0.5 s of iterations: the budget
            # per engine call shrinks when a single iteration is slow (measured on the run so far)
            budget = max_kkt - drv.j
            if drv.k >= 2 * drv.period:
                per_iter = (time.time() - t0) / drv.k
                budget = min(budget, max(1, int(0.5 / max(per_iter, 1e-9))))
            if eng.comm is not None:                                        # every rank must take the same steps: rank 0 decides
                flag = torch.tensor([int(expired), int(budget)], dtype=torch.int64, device=eng.device)
                eng.comm.dist.broadcast(flag, 0, group=eng.comm.group)
                expired, budget = bool(int(flag[0])), int(flag[1])
            if expired:
                status = STATUS_TIME_LIMIT
                if verbose:
                    print("Time limit exceeded")
                break
            drv.advance(budget)
            if drv.infeasible:
                break
        if drv.infeasible:                                                  # pdhg.py:94-100: leave at once with c'x
            status = drv.infeasible
            drv.res = eng.kkt(N.CUR, drv.omega)
            break
        if status == STATUS_TIME_LIMIT:
            break
        if drv.n == n_before:        # left the inner loop through the KKT-pass cap (pdhg.py:67 -> :148)
            drv.after_restart(None)
        if drv.solved:                                                      # pdhg.py:173-177
            status = STATUS_SOLVED
            if verbose:
                print(f"Converged at iteration {drv.k} restart loop {drv.n}")
            break
    final = N.AVG if halpern and drv.tt > 0 else N.CUR     # (Halpern between restarts: the candidate, which is inside the bounds)
    x_local, _ = eng.get_iterate(final)
    if report is not None:
        report.update(eng.report(final, unscaled=bool(precondition), omega=drv.omega))
        report.update(q_norm=float(drv.q_norm), c_norm=float(drv.c_norm))      # as the exit test took them (pdhg.py:19-20)
    eng.synchronize()                                  # the reference reads its clock without a sync (Q10)
    prim_obj = float(drv.res["p"]) if drv.res is not None else float("nan")
    return x_local, prim_obj, drv.k, drv.n, drv.j, status, time.time() - t0 + time_used


def pdlp_algorithm(K, m_ineq, c, q, l, u, device=None, max_kkt=100_000, tol=1e-4, verbose=True, restart_period=40,
                   precondition=False, primal_update=False, adaptive=False, data_precond=None, infeasibility_detect=False,
                   infeas_tol=1e-4, time_limit=3600, time_used=0, x_init=None, y_init=None, *, b0=None, sigma=None,
                   seed=None, trace=None, comm=None, precision=None, adaptive_retry=False, report=None,
                   halpern=False, q_upper=None, quad_diag=None, halpern_restart="kkt", quad_matrix=None, quad_norm=None,
                   quad_step="fixed"):
    """Drop-in for the reference's ``pdlp_algorithm`` (primal_dual_hybrid_gradient.py:7) on one MI355X.

    ``K`` may be a dense / COO torch tensor (as the reference takes), a scipy sparse matrix or a
    ``CsrPair``.  With ``precondition=True`` pass the scaled problem and ``data_precond`` as returned by
    ``ruiz_precondition`` (its first two entries ``D_col, D_row`` are what is used; with ``pock_chambolle=True`` there
    they hold the Pock-Chambolle pass as well, and nothing here changes).  ``b0`` / ``sigma`` /
    ``seed`` pin the power-iteration start the reference leaves to an unseeded RNG.
    Returns ``(x, prim_obj, k, n, j, status, total_time)``; ``x`` is an (n,1) tensor and, like the
    reference's (quirk Q4), the SCALED iterate when preconditioned.

    ``adaptive_retry`` (with ``adaptive``; default off = the live package's behaviour, quirk Q1): the adaptive step as it was
    meant -- a rejected trial is repeated from the same iterate with the shrunk step size until one is accepted
    (/root/reference/enhancements/test_ass.py:322-363) instead of being kept.

    ``precision="mixed"``: float64 vectors, products and sums over a matrix held in float32 -- for tolerances below float32
    resolution (the reference is float32 only) on matrices whose entries are float32 numbers (checked); 8 instead of 12 bytes
    per non-zero, and the iterations run on the float32 kernels over difference vectors (delta mode, include/pdlp_hip.h).
    ``c, q, l, u`` are taken in float64.  A matrix that is NOT float32-valued (any float64 ``K``, a Ruiz-scaled one with
    ``precondition=True``) works too, sharded included: the iterations then run on its float32 rounding and the anchors of delta
    mode and the termination test are evaluated with the true float64 matrix after every restart.

    ``report``: a dict that receives the solution report of the returned iterate -- ``y``, ``reduced_costs``, ``row_activity``
    (full (m,1) / (n,1) tensors) and ``pr, dr, gap, p, d_adj, kkt`` (helpers.py:53-108), of the ORIGINAL problem when
    ``precondition`` (un-like ``x``) -- for every exit status; ``q_norm``, ``c_norm``: the norms check_termination was given
    (pdhg.py:19-20,173: of the ``q`` and ``c`` passed in, i.e. of the scaled vectors when ``precondition``).

    ``halpern`` (default off; the reference has no counterpart): the restarted, reflected Halpern iteration instead of averaged
    PDHG -- fixed step, the restart rules and the primal weight unchanged, evaluated at the candidate (one PDHG step from the
    Halpern iterate); see ``PdhgDriver`` and DESIGN.md 4.2.  Works with ``precondition``, ``primal_update`` and ``x_init`` /
    ``y_init``; ``ValueError`` together with ``adaptive``, ``adaptive_retry``, ``infeasibility_detect``, ``precision="mixed"`` or
    ``comm``.  ``halpern_restart`` (default "kkt": the sentence above): "fixed_point" restarts on the fixed-point residual
    ``||z - T(z)||_P`` of the Halpern iterate instead of the candidate's KKT error -- the criterion of the rHPDHG papers; a check then
    costs one product and no KKT pass (``PdhgDriver``).  ``ValueError`` (before any device work) for another value
    and for "fixed_point" without ``halpern``.

    ``q_upper`` (length m, default None): two-sided rows ``q_i <= (K x)_i <= q_upper_i`` on the inequality rows, entered once
    (``+inf``: a one-sided row; ``== q_i``: behaves as an equality row; on equality rows ``+inf`` or ``q_i``, ignored); the sign
    of ``y`` says which side is active (``y_i > 0`` the lower, ``y_i < 0`` the upper); with ``precondition`` pass the scaled one
    (``Scaling.scale``).  DESIGN.md 4.3.  Works with ``precondition``, ``primal_update``, ``adaptive``, ``halpern`` and ``x_init`` /
    ``y_init`` in float32 and float64; ``ValueError`` (before any device work) for a malformed ``q_upper`` and together with
    ``precision="mixed"``, ``comm``, ``infeasibility_detect`` or ``adaptive_retry``.

    ``quad_diag`` (length n, default None; the reference has no counterpart): the objective becomes ``c'x + 1/2 sum_j d_j x_j^2`` with
    ``d = quad_diag >= 0``: the primal half-step divides by ``1 + tau d_j`` before the clamp, the gradient of the KKT
    pass is ``c + D x - K'y``, the returned objective is the quadratic one and the report's dual objective carries ``-1/2 x'Dx``;
    with ``precondition`` pass the scaled diagonal (``Scaling.scale(..., quad_diag=)``: ``d D_col^2``).  Works with ``precondition``,
    ``primal_update``, ``adaptive``, ``halpern``, ``q_upper`` and ``x_init`` / ``y_init`` in float32 and float64; ``ValueError`` (before
    any device work) for a malformed vector and together with ``precision="mixed"``, ``comm``, ``infeasibility_detect`` or
    ``adaptive_retry``.

    ``quad_matrix`` (n x n, default None; the reference has no counterpart): the objective becomes ``c'x + 1/2 x'Qx`` with ``Q``
    sparse, symmetric and positive semidefinite -- the last is the caller's duty, ``quad.check_quad_matrix`` checks the rest (DESIGN.md
    4.5).  The iteration takes the linearised step (the gradient ``Qx`` joins ``c`` in the primal half-step) with the fixed step
    ``rules.qp_eta``, which the driver sets anew whenever a restart changes the primal weight; ``quad_norm`` overrides the power
    iteration's estimate of ``||Q||_2`` as ``sigma`` overrides that of ``||K||_2``.  The returned objective is the quadratic one, the
    report's dual objective carries ``-1/2 x'Qx`` and its reduced costs are ``project_lambda_box(c + Qx - K'y)``; with
    ``precondition`` pass the scaled matrix (``Scaling.scale(..., quad_matrix=)``: ``D_col Q D_col``).  Works with ``precondition``,
    ``primal_update``, ``q_upper``, ``quad_diag`` and ``x_init`` / ``y_init`` in float32 and float64; ``ValueError`` (before any device
    work) for a malformed matrix and together with ``adaptive``, ``halpern``, ``adaptive_retry``, ``infeasibility_detect``,
    ``precision="mixed"`` or ``comm``.  ``quad_step="adaptive"`` (default "fixed"): the same linearised step under an adaptive step
    size -- the reference's rule (step.py:91-115) with the curvature measured along the step in its denominator,
    ``eta_bar = (omega ||dx||^2 + ||dy||^2 / omega) / (2 |dy'K dx| + max(dx'Q dx, 0))``, at the same three products per iteration
    (DESIGN.md 4.5.1); it starts from ``rules.qp_eta`` and composes with everything ``quad_matrix`` composes with.  ``ValueError``
    (before any device work) for another value, without ``quad_matrix``, and together with anything ``quad_matrix`` refuses
    (``adaptive`` included: that switch is the LP's rule).

    ``comm`` (a ``Comm``, or ``True`` for the default ``torch.distributed`` group): every rank calls with the SAME
    full problem and the same ``seed``/``b0``; each keeps its row blocks of K and K', the iterations exchange
    ``xbar`` and ``y`` over RCCL, and every rank returns the full solution.
    """
    from .distributed import gather_report, gather_solution, shard_engine, start_blocks
    check_halpern_restart(halpern_restart, halpern)
    check_quad_step(quad_step, quad_matrix is not None)
    check_composition(halpern=halpern, q_upper=q_upper is not None, quad_diag=quad_diag is not None,
                      quad_matrix=quad_matrix is not None, adaptive=adaptive, adaptive_retry=adaptive_retry, infeasibility_detect=infeasibility_detect, mixed=precision is not None, comm=comm not in (None, False))
    q_upper = check_row_upper(q, q_upper, m_ineq)
    quad_diag = check_quad_diag(quad_diag, torch.as_tensor(c).numel())
    quad_matrix = check_quad_matrix(quad_matrix, torch.as_tensor(c).numel())
    device = resolve_device(device)
    Kp = CsrPair.from_any(K, device=device)
    dtype = Kp.dtype
    vec_dtype = None
    exact_K = None
    if is_mixed(precision):
        from .engine import values_are_float32
        if not (values_are_float32(Kp.val) and values_are_float32(Kp.t_val)):
            # any float64 matrix (e.g. a Ruiz-scaled one): the iterations run on its float32 ROUNDING (they only multiply
            # difference vectors), the anchors and the termination test use the true matrix (engine.py, `exact`; sharded: every
            # rank holds the same full matrix here, so all ranks take this branch together)
            exact_K = Kp
        Kp = Kp.to(dtype=torch.float32)
        dtype = vec_dtype = torch.float64
    d_col, d_row = precond_factors(precondition, data_precond)
    if comm is True:
        comm = Comm()
    sharded = comm is not None and comm.world > 1
    if sharded:
        if seed is None and b0 is None and sigma is None:
            seed = 0                                   # the ranks must draw the same power-iteration start
        eng = shard_engine(Kp, c, q, l, u, m_ineq, comm, d_col=d_col, d_row=d_row, vec_dtype=vec_dtype, exact=exact_K)    # blocks balanced by non-zeros
        x_init, y_init = start_blocks(eng, x_init, y_init, Kp.n, Kp.m)
        if b0 is not None:
            b0 = eng.part.pad_cols(as_vec(b0, Kp.n, device, torch.float32))
        verbose = verbose and comm.rank == 0
    else:
        eng = PdlpEngine.from_full(Kp, c, q, l, u, m_ineq, d_col=d_col, d_row=d_row, vec_dtype=vec_dtype, exact=exact_K, q_upper=q_upper,
                                   **({} if quad_diag is None else dict(quad_diag=quad_diag)),
                                   **({} if quad_matrix is None else dict(quad_matrix=quad_matrix)))
    x, obj, k, n, j, status, total = run_pdlp(
        eng, max_kkt=max_kkt, tol=tol, verbose=verbose, restart_period=restart_period, precondition=precondition,
        primal_update=primal_update, adaptive=adaptive, time_limit=time_limit, time_used=time_used, x_init=x_init, y_init=y_init,
        b0=b0, sigma=sigma, seed=seed, trace=trace, infeasibility_detect=infeasibility_detect, infeas_tol=infeas_tol,
        adaptive_retry=adaptive_retry, report=report, halpern=halpern, halpern_restart=halpern_restart,
        **({} if quad_matrix is None else dict(quad_norm=quad_norm, quad_step=quad_step)))
    if report is not None:
        report.update(gather_report(eng, report, Kp.n, Kp.m))
    return gather_solution(eng, x, Kp.n).view(-1, 1), obj, k, n, j, status, total
