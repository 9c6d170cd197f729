"""The host-side rules of the reference's ``pdlp_algorithm`` (``/root/reference/PDLP/primal_dual_hybrid_gradient.py:7-181``,
``helpers.py:84-128``, ``enhancements.py:73-78``): when to restart, with which primal weight, and when to stop.

``StreamQueue`` is the bookkeeping of a family streamed through the columns of a batch (``pdlp_algorithm_batch(slots=...)``).

Pure numpy, no torch and no native library.  Every function takes scalars or arrays of any shape and returns the kind of thing it
was given: ``PdhgDriver`` (solver.py) calls them with its scalars, ``BatchDriver`` (batch.py) with its ``[B]`` arrays.  Every
intermediate is rounded to the working precision ``t`` (np.float32 / np.float64; ``t(v)`` of an array is an array of that type).
"""
from __future__ import annotations

import numpy as np

BETA = (0.2, 0.8, 0.36)                                       # pdhg.py:28: sufficient, necessary, artificial
STATUS_KKT_LIMIT = "Unsolved (KKT passes limit exceeded)"     # pdhg.py:51
STATUS_TIME_LIMIT = "Unsolved (Time limit exceeded)"          # pdhg.py:71
STATUS_SOLVED = "Solved"                                      # pdhg.py:174


def np_type(dtype):
    """the numpy scalar type of a working precision given as a torch or numpy dtype"""
    return np.float32 if str(dtype).endswith("float32") else np.float64


def kkt_error(res: dict, omega, t=np.float32):
    """KKT_error (helpers.py:98-108) of known residuals under ``omega``: the residuals do not depend on the primal weight, so a
    change of omega (pdhg.py:153) is a re-weighting of numbers already there"""
    w2 = t(omega) * t(omega)
    pr, dr, gap = t(res["pr"]), t(res["dr"]), t(res["gap"])
    return np.sqrt(w2 * (pr * pr) + (dr * dr) / w2 + gap * gap)


def kkt_from_sums(red, omega, t=np.float32) -> dict:
    """helpers.py:84-106 from the six sums of a KKT pass (``red[..., 6]`` in the order of PDLP_BUF_RED) -- the library's kkt_finish"""
    red = np.asarray(red)
    p, d, lp, un = (t(red[..., i]) for i in (3, 5, 1, 2))
    adj = d + lp + un
    res = dict(pr=t(np.sqrt(red[..., 4])), dr=t(np.sqrt(red[..., 0])), gap=adj - p, p=p, d_adj=adj)
    res["kkt"] = kkt_error(res, omega, t)
    return res


def terminated(res: dict, q_norm, c_norm, tol, t=np.float32):
    """check_termination (helpers.py:110-128); the gap is signed (reference quirk Q2)"""
    pr, dr, gap, p, adj, tol = (t(v) for v in (res["pr"], res["dr"], res["gap"], res["p"], res["d_adj"], tol))
    c1 = pr <= tol * (1 + q_norm)
    c2 = dr <= tol * (1 + c_norm)
    c3 = gap <= tol * (1 + abs(p) + abs(adj))
    return c1 & c2 & c3


def previous_kkt_matters(kkt_cur, kkt_avg, kkt_first, t=np.float32):
    """whether KKT_previous can change ``restart_decision``: it only enters the "necessary" test (pdhg.py:135), which is reached
    when the sufficient one fails and whose first half does not need it"""
    kc, ka, kf = t(kkt_cur), t(kkt_avg), t(kkt_first)
    k_min = t(np.where(ka < kc, ka, kc))
    return ~(k_min <= t(BETA[0]) * kf) & (k_min <= t(BETA[1]) * kf)


def restart_decision(kkt_cur, kkt_avg, kkt_prev, kkt_first, tt, k, j, live=True, max_kkt=np.inf, t=np.float32) -> dict:
    """The restart decision of one check (pdhg.py:115-146) and the KKT-pass cap (pdhg.py:54,67).

    ``kkt_*`` are the KKT errors at the current, averaged and previous iterates, ``kkt_first`` the one of the last restart point
    (0 before the first restart: the first check can only restart artificially), ``tt`` the iterations since the last restart,
    ``k`` the iteration count, ``j`` the KKT-pass count AFTER the check's three passes.  Returns ``crit`` (-1 none, 0 sufficient,
    1 necessary, 2 artificial), ``use_avg``, ``capped`` (no restart, and ``j`` has reached ``max_kkt``: the reference leaves the
    inner loop and continues at pdhg.py:148 from the current iterate) and ``action`` (0 keep, 1 restart at the current iterate,
    2 at the average).  Dead LPs (``live`` false) get -1 / False / 0."""
    kc, ka, kp, kf = t(kkt_cur), t(kkt_avg), t(kkt_prev), t(kkt_first)
    live = np.asarray(live, dtype=bool)
    k_min = np.where(ka < kc, ka, kc)                          # Python's min(KKT_current, KKT_average) of pdhg.py:124
    use_avg = (kc >= ka) & live
    suff = k_min <= t(BETA[0]) * kf
    nec = (k_min <= t(BETA[1]) * kf) & (k_min > kp)
    art = np.asarray(tt, dtype=np.float64) >= BETA[2] * np.asarray(k, dtype=np.float64)      # in float64, like the int * float there
    crit = np.where(live, np.where(suff, 0, np.where(nec, 1, np.where(art, 2, -1))), -1)
    restart = crit >= 0
    capped = live & ~restart & (np.asarray(j) >= max_kkt)
    action = np.where(restart, np.where(use_avg, 2, 1), np.where(capped, 1, 0)).astype(np.int32)
    return dict(crit=crit[()], use_avg=use_avg[()], capped=capped[()], action=action[()])


def fixed_point_error(dx2, cross, dy2, eta, omega):
    """The fixed-point residual ``||z - T(z)||_P`` of a Halpern iterate from the three sums of ``pdlp_halpern_fixed_point``
    (``||dx||^2``, ``dx'K'dy``, ``||dy||^2`` with ``dz = z - T(z)``) under the step's metric ``P = [[1/tau, -K'], [-K, 1/sigma]]``,
    ``tau = eta/omega``, ``sigma = eta omega``:  ``r^2 = (omega/eta) ||dx||^2 - 2 dx'K'dy + ||dy||^2 / (eta omega)``.
    Formed in float64 whatever the working precision (the sums are float64); a negative ``r^2`` -- rounding, when the three terms
    cancel -- is clipped at 0."""
    dx2, cross, dy2, eta, omega = (np.asarray(v, dtype=np.float64) for v in (dx2, cross, dy2, eta, omega))
    r2 = (omega / eta) * dx2 - 2.0 * cross + dy2 / (eta * omega)
    return np.sqrt(np.maximum(r2, 0.0))[()]


def fixed_point_restart_decision(r, r_prev, r0, tt, k, j=0, live=True, max_kkt=np.inf, t=np.float32) -> dict:
    """The restart decision of one check of the Halpern mode under ``halpern_restart="fixed_point"``: ``restart_decision``'s three
    criteria with the fixed-point residual in the place of the KKT error.

    ``r`` is the residual of the last iteration (``fixed_point_error``), ``r_prev`` the one at the previous check of this restart
    period (``inf`` at the first check), ``r0`` the one at the restart point (of the first iteration after the restart), ``tt`` the
    iterations since the last restart, ``k`` the iteration count.  Sufficient: ``r <= BETA[0] r0``; necessary: ``r <= BETA[1] r0``
    and ``r > r_prev``; artificial: ``tt >= BETA[2] k``; in that order.  Returns the dict of ``restart_decision``: a restart always
    adopts the candidate, so ``use_avg`` is true and ``action`` is 2 whenever ``crit >= 0``."""
    rc, rp, rf = t(r), t(r_prev), t(r0)
    live = np.asarray(live, dtype=bool)
    suff = rc <= t(BETA[0]) * rf
    nec = (rc <= t(BETA[1]) * rf) & (rc > rp)
    art = np.asarray(tt, dtype=np.float64) >= BETA[2] * np.asarray(k, dtype=np.float64)
    crit = np.where(live, np.where(suff, 0, np.where(nec, 1, np.where(art, 2, -1))), -1)
    restart = crit >= 0
    capped = live & ~restart & (np.asarray(j) >= max_kkt)
    action = np.where(restart, 2, np.where(capped, 1, 0)).astype(np.int32)
    return dict(crit=crit[()], use_avg=restart[()], capped=capped[()], action=action[()])


def start_eta(sigma, t=np.float32):
    """pdhg.py:22: the first step size from the estimate of ||K||_2"""
    return t(0.9) / t(sigma)


def qp_eta(sigma, quad_norm, omega, t=np.float32):
    """The fixed step of the linearised iteration for ``min c'x + 1/2 x'Qx`` (``quad_matrix``): with ``s`` the estimate of ``||K||_2``,
    ``L`` that of ``||Q||_2`` and ``tau = eta/omega``, ``sigma = eta omega`` the step converges for
    ``1/tau - sigma ||K||^2 >= ||Q||/2``, that is ``omega/eta - eta omega s^2 >= L/2``; the largest such ``eta`` is the positive root
    of ``omega s^2 eta^2 + (L/2) eta - omega = 0``, and the step is 0.9 of it -- the safety ``start_eta`` has --

        ``eta = 0.9 (-L/2 + sqrt(L^2/4 + 4 omega^2 s^2)) / (2 omega s^2)``,

    formed in double and rounded ONCE to ``t``.  At 0.9 of the root the condition holds with a factor above 1.11 to spare (the left
    side is decreasing in ``eta``), which an under-estimate of ``L`` by the power iteration may use up.  ``L == 0`` (a ``Q`` without
    stored entries) is DEFINED as ``start_eta(s, t)``: the LP's step, bit for bit.  Unlike the LP's, the step depends on ``omega``:
    the driver sets it anew after every restart that changes the primal weight."""
    if float(quad_norm) == 0.0:
        return start_eta(sigma, t)
    s, L, w = np.float64(sigma), np.float64(quad_norm), np.float64(omega)
    # the same root with the conjugate in the denominator, 2 omega / (L/2 + sqrt(L^2/4 + 4 omega^2 s^2)): the difference above
    # cancels to nothing in double once L is large against omega s
    return t(0.9 * (2.0 * w) / (0.5 * L + np.sqrt(0.25 * L * L + 4.0 * w * w * s * s)))


def start_omega(q_norm, c_norm, t=np.float32):
    """pdhg.py:23: the first primal weight ||c|| / ||q||, 1 when either norm is (nearly) zero"""
    q_norm, c_norm = t(q_norm), t(c_norm)
    with np.errstate(divide="ignore", invalid="ignore"):
        return t(np.where((q_norm > 1e-6) & (c_norm > 1e-6), c_norm / q_norm, t(1.0)))


def halpern_weights(t_iter, dtype=np.float32):
    """``(a, b) = ((t+1)/(t+2), 1/(t+2))`` of Halpern iteration number ``t_iter`` since the last restart (0 for the first): the
    new iterate is ``a * reflected point + b * anchor``.  Both are formed in float64 and rounded once to the working precision
    ``dtype`` (a torch or numpy dtype, or a numpy scalar type) -- what ``pdlp_halpern_iterate`` hands its kernels"""
    t = np_type(getattr(dtype, "__name__", dtype))
    t2 = np.float64(int(t_iter) + 2)
    return t(np.float64(int(t_iter) + 1) / t2), t(np.float64(1.0) / t2)


def primal_weight(dx2, dy2, omega, smooth_theta=0.5, t=np.float32):
    """primal_weight_update (enhancements.py:73-78) given the two squared restart distances.

    Array input is evaluated element by element (np.vectorize is a Python loop): numpy may use a SIMD ``log`` / ``exp`` for float64
    arrays whose last bit can differ from the scalar routine's, and an LP's primal weight must not depend on its batch."""
    if np.ndim(dx2) or np.ndim(dy2) or np.ndim(omega):
        return np.vectorize(lambda a, b, w: primal_weight(a, b, w, smooth_theta, t), otypes=[t])(dx2, dy2, omega)
    dxn, dyn = t(np.sqrt(dx2)), t(np.sqrt(dy2))
    if dxn > 0 and dyn > 0:
        # every intermediate is rounded to the working precision, as the reference's 0-dim tensors are;
        # log / exp are evaluated in double and rounded once (same definition as oracle/pdlp_oracle_impl.inc)
        lr = t(np.log(np.float64(t(dyn / dxn))))
        lw = t(np.log(np.float64(t(omega))))
        return t(np.exp(np.float64(t(t(smooth_theta) * lr) + t((t(1) - t(smooth_theta)) * lw))))
    return t(omega)


class StreamQueue:
    """Which LP of a family of ``B`` runs in which of ``slots`` columns, and when (``pdlp_algorithm_batch(slots=...)``).

    The LPs wait in index order.  A column is free until ``admit`` gives it the next waiting LP and again once ``retire`` has taken
    its LP out.  Admission is allowed only when the batch's iteration count ``k_global`` is a multiple of ``period``: every LP's
    restart checks fall on multiples of the period of its OWN count (pdhg.py:115), so an LP that enters at a check of the batch
    meets every later check of the batch at a check of its own -- the control flow of a batch that started with it.
    ``column``, ``admitted_at``, ``retired_at`` (``[B]``; -1: never) are the schedule of the run."""

    def __init__(self, B: int, slots: int, period: int):
        if B < 1 or slots < 1 or period < 1:
            raise ValueError("a family, the columns and the period are all at least 1")
        self.B, self.slots, self.period = int(B), int(slots), int(period)
        self.next = 0                                             # the first LP still waiting
        self.lp = np.full(self.slots, -1, np.int64)               # column -> LP, -1 free
        self.column = np.full(self.B, -1, np.int64)
        self.admitted_at = np.full(self.B, -1, np.int64)
        self.retired_at = np.full(self.B, -1, np.int64)

    def waiting(self) -> int:
        return self.B - self.next

    def occupied(self) -> np.ndarray:
        return np.flatnonzero(self.lp >= 0)

    def free(self) -> np.ndarray:
        return np.flatnonzero(self.lp < 0)

    def may_admit(self, k_global: int) -> bool:
        return int(k_global) % self.period == 0

    def next_boundary(self, k_global: int) -> int:
        """the first count >= ``k_global`` at which admission is allowed"""
        return -(-int(k_global) // self.period) * self.period

    def admit(self, k_global: int):
        """the free columns, lowest first, take the next waiting LPs: ``(cols, ids)`` (empty when nothing waits or nothing is free)"""
        if not self.may_admit(k_global):
            raise ValueError(f"admission at k = {k_global}: not a multiple of the restart period {self.period}")
        cols = self.free()[:self.waiting()]
        ids = np.arange(self.next, self.next + cols.size, dtype=np.int64)
        self.lp[cols] = ids
        self.column[ids] = cols
        self.admitted_at[ids] = int(k_global)
        self.next += int(cols.size)
        return cols, ids

    def retire(self, cols, k_global: int) -> np.ndarray:
        """the LPs of ``cols`` leave; their ids"""
        cols = np.asarray(cols, np.int64).reshape(-1)
        ids = self.lp[cols].copy()
        if (ids < 0).any():
            raise ValueError(f"columns {cols[ids < 0].tolist()} hold no LP")
        self.retired_at[ids] = int(k_global)
        self.lp[cols] = -1
        return ids

    def never_admitted(self) -> np.ndarray:
        """the LPs still waiting (at a time-limit cut: they come back with k = 0)"""
        return np.arange(self.next, self.B, dtype=np.int64)

    def schedule(self) -> dict:
        return dict(column=self.column.copy(), admitted_at=self.admitted_at.copy(), retired_at=self.retired_at.copy())
