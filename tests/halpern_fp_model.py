"""The Halpern mode under ``halpern_restart="fixed_point"`` in float64 numpy with dense products: a numpy engine with
``halpern_fixed_point`` that ``run_pdlp`` can drive and that records the driver's calls, and the whole driver stated straight down
(``fixed_point_driver_model``), which also reports how far every threshold comparison of its run was from flipping.  Over
``tests/ranged_model.RangedModel`` (two-sided rows) or ``tests/quad_model.QuadModel``.  Needs no GPU."""
import numpy as np

from tests.ranged_model import RangedModelEngine
from torchpdlp_amd import rules


def fixed_point_sums(A, zx, zy, xc, yc):
    """``(||dx||^2, dx'A'dy, ||dy||^2)`` with ``dx = zx - xc``, ``dy = zy - yc``: what ``pdlp_halpern_fixed_point`` leaves in the
    first three sums"""
    dx, dy = zx - xc, zy - yc
    return float(dx @ dx), float(dx @ (A.T @ dy)), float(dy @ dy)


class FixedPointModelEngine(RangedModelEngine):
    """``RangedModelEngine`` with the new call; ``calls`` lists what the driver asked for, in order"""

    def __init__(self, model, q_upper=True):
        super().__init__(model, q_upper=q_upper)
        self.calls = []
        self.zx = self.zy = None                          # the iterate before the last Halpern iteration (N.PREV of the handle)

    def halpern_iterate(self, iters):
        self.calls.append(("halpern_iterate", int(iters)))
        for _ in range(int(iters)):
            self.zx, self.zy = self.x, self.y
            super().halpern_iterate(1)

    def halpern_fixed_point(self):
        self.calls.append(("halpern_fixed_point",))
        assert self.zx is not None, "no Halpern iteration since the last restart / set_iterate: the library returns PDLP_ERR_STATE"
        return fixed_point_sums(self.mo.A, self.zx, self.zy, self.xa, self.ya)

    def iterate(self, iters, adaptive):
        raise AssertionError("the Halpern mode never takes a PDHG iteration")

    flush_average = compute_average = iterate

    def kkt(self, which, omega, unscaled=False):
        self.calls.append(("kkt", int(which)))
        return super().kkt(which, omega, unscaled)

    def restart(self, which):
        self.calls.append(("restart", int(which)))
        super().restart(which)
        self.zx = self.zy = None

    def set_iterate(self, x, y):
        super().set_iterate(x, y)
        self.zx = self.zy = None

    def restart_distance(self):
        self.calls.append(("restart_distance",))
        return super().restart_distance()

    def mark_restart_point(self):
        self.calls.append(("mark_restart_point",))
        super().mark_restart_point()


def _margin(a, b):
    """how far ``a <= b`` (or ``a > b``) is from flipping, relative to the larger side (inf when a side is infinite or both are 0)"""
    a, b = float(a), float(b)
    if not (np.isfinite(a) and np.isfinite(b)) or max(abs(a), abs(b)) == 0.0:
        return np.inf
    return abs(a - b) / max(abs(a), abs(b))


def fixed_point_driver_model(mo, sigma, tol, primal_update=True, period=40, max_kkt=1_000_000):
    """The method, straight down, in float64: the reflected Halpern iteration with the fixed step ``0.9 / sigma``, ``r0`` after the
    first iteration of a restart period, a check of the fixed-point residual every ``period`` iterations with the three criteria in
    their order, the restart at the candidate, the primal weight, the KKT pass at the restart point and the termination test.
    -> dict(x, k, n, j, restarts [(crit, tt, 1)], status, margin): ``margin`` is the smallest relative distance from equality over
    every comparison with a threshold the run made (residual against 0.2 r0, 0.8 r0 and the previous residual; the three
    termination tests at every restart) -- the artificial criterion compares integers in float64 on the host in the driver and here
    alike, so it cannot differ."""
    t = np.float64
    q_norm, c_norm = t(mo.norm_q()), t(np.linalg.norm(mo.c))
    eta, omega = rules.start_eta(sigma, t), rules.start_omega(q_norm, c_norm, t)
    x, y = np.zeros(mo.n), np.zeros(mo.m)
    k = n = j = 0
    restarts, margin = [], np.inf
    while j < max_kkt:
        xa, ya, tt, r_prev, r0 = x.copy(), y.copy(), 0, np.inf, None
        while True:
            zx, zy = x, y
            x, y, xc, yc = mo.halpern_step(x, y, xa, ya, tt, float(eta) / float(omega), float(eta) * float(omega))
            k, tt, j = k + 1, tt + 1, j + 1
            if tt == 1:
                r0, j = rules.fixed_point_error(*fixed_point_sums(mo.A, zx, zy, xc, yc), eta, omega), j + 1
            if tt % period:
                continue
            r, j = rules.fixed_point_error(*fixed_point_sums(mo.A, zx, zy, xc, yc), eta, omega), j + 1
            margin = min(margin, _margin(r, rules.BETA[0] * r0), _margin(r, rules.BETA[1] * r0), _margin(r, r_prev))
            crit = 0 if r <= rules.BETA[0] * r0 else 1 if (r <= rules.BETA[1] * r0 and r > r_prev) else \
                2 if tt >= rules.BETA[2] * k else -1
            r_prev = r
            if crit >= 0:
                restarts.append((crit, tt, 1))
                x, y = xc, yc
                break
        n += 1
        if primal_update:
            omega = rules.primal_weight(float(np.sum((xa - x) ** 2)), float(np.sum((ya - y) ** 2)), omega, 0.5, t)
        res = mo.kkt(x, y, float(omega))
        j += 2
        margin = min(margin, _margin(res["pr"], tol * (1 + q_norm)), _margin(res["dr"], tol * (1 + c_norm)),
                     _margin(res["gap"], tol * (1 + abs(res["p"]) + abs(res["d_adj"]))))
        if rules.terminated(res, q_norm, c_norm, tol, t):
            return dict(x=x, k=k, n=n, j=j, restarts=restarts, status=rules.STATUS_SOLVED, margin=margin)
    return dict(x=x, k=k, n=n, j=j, restarts=restarts, status=rules.STATUS_KKT_LIMIT, margin=margin)


def expected_calls(restarts, checks, period, primal_update):
    """the engine calls of a run with ``checks`` restart checks, the restarts of ``restarts`` (the model's list) and a solve that
    ends at the last restart: ``halpern_iterate(1), halpern_fixed_point, halpern_iterate(period - 1), halpern_fixed_point, ...``"""
    from torchpdlp_amd import _native as N
    out, tt, left = [], 0, list(restarts)
    for _ in range(checks):
        if tt == 0:
            out += [("halpern_iterate", 1), ("halpern_fixed_point",)] + ([("halpern_iterate", period - 1)] if period > 1 else [])
        else:
            out += [("halpern_iterate", period)]
        tt += period
        out += [("halpern_fixed_point",)]
        if left and left[0][1] == tt:
            left.pop(0)
            out += [("restart", N.AVG)] + ([("restart_distance",)] if primal_update else []) + [("mark_restart_point",), ("kkt", N.CUR)]
            tt = 0
    assert not left
    return out
