"""The adaptive step of the sparse quadratic objective (``quad_step="adaptive"``, pdlp_objective_iterate) in float64 numpy with dense
products: ``GeneralQuadModel`` (tests/qp_model.py) with the step-size rule extended by the measured curvature ``dx'Q dx``, and a numpy
engine over it that ``run_pdlp`` can drive with ``quad_step="adaptive"``.  The model tests/test_quad_adaptive_host.py and
tests/test_gpu_quad_adaptive.py compare against.  Needs no GPU."""
from types import SimpleNamespace

import numpy as np

from tests.qp_model import GeneralQuadEngine, GeneralQuadModel


class AdaptiveQuadModel(GeneralQuadModel):
    """``GeneralQuadModel`` whose ``adaptive_step`` bounds the step by ``2 |dy'K dx| + max(dx'Q dx, 0)``.  A large ``Q`` is multiplied
    through a sparse copy (the arrow matrix of the table is 2600 x 2600 with 7798 entries: the dense product is most of a run's
    time); a small one stays dense, in ``GeneralQuadModel``'s order of additions -- the 1e-8 rows of the table end at the floor of
    float64, where the number of rejected trials follows that order."""

    def __init__(self, A, m_ineq, c, q, l, u, Q=None, d=None, qu=None):
        import scipy.sparse as sp
        super().__init__(A, m_ineq, c, q, l, u, Q, d, qu)
        self.Qs = sp.csr_matrix(self.Q) if self.n > 1000 else self.Q

    def grad(self, x):
        return self.c + self.Qs @ x

    def half(self, x):
        return 0.5 * float(x @ (self.Qs @ x)) + 0.5 * float(np.sum(self.d * x * x))

    def rule(self, x, y, eta, omega, k, curvature=True):
        """one trial of the linearised step from (x, y) and the rule's numbers -> namespace(x, y: the trial, kept whatever the
        verdict; g, g_new: c + Q x of the old and of the new x; nx2, ny2, dykdx: the three sums of the LP's rule; curv = dx'Q dx;
        den = 2 dy'K dx; eta_bar, accepted, eta_next; weight: the step size the trial used, eta when it was accepted and eta_next
        when not, step.py:110-115); ``curvature=False``: the LP's eta_bar at the same point"""
        xc, yc, _, _ = self.step(x, y, eta / omega, eta * omega)
        dx, dy = xc - x, yc - y
        g, gn = self.grad(x), self.grad(xc)
        nx2, ny2, dykdx = float(dx @ dx), float(dy @ dy), float(dy @ (self.A @ dx))
        curv = float(dx @ (self.Qs @ dx))
        den = 2 * dykdx
        den_abs = abs(den) + (max(curv, 0.0) if curvature else 0.0)
        if den_abs != 0:
            eta_bar = (omega * nx2 + ny2 / omega) / den_abs
            t1 = (1 - (k + 1) ** (-0.3)) * eta_bar
        else:
            eta_bar = t1 = np.inf
        eta_next = min(t1, (1 + (k + 1) ** (-0.6)) * eta)
        accepted = eta <= eta_bar
        return SimpleNamespace(x=xc, y=yc, g=g, g_new=gn, nx2=nx2, ny2=ny2, dykdx=dykdx, curv=curv, den=den, eta_bar=eta_bar,
                               accepted=bool(accepted), eta_next=eta_next, weight=eta if accepted else eta_next)

    def adaptive_step(self, x, y, eta, omega, k):
        """``RangedModel.adaptive_step`` with the curvature in the denominator -> (x', y', eta')"""
        r = self.rule(x, y, eta, omega, k)
        return r.x, r.y, r.eta_next


class AdaptiveQuadEngine(GeneralQuadEngine):
    """``GeneralQuadEngine`` with ``objective_iterate``: what solver.py uses of PdlpEngine under ``quad_step="adaptive"``.  The
    averages are ``QuadModelEngine.iterate``'s for the adaptive step (``weights="next"``: an iterate is weighed with the step size
    the rule left behind) -- the convention of the table in DESIGN.md 4.5.1 -- or the library's (``weights="used"``: with the step size its
    trial used, ``eta`` when accepted and ``eta'`` when not, step.py:110-115).  The table's seed-1 rows come out the same under
    either; 600 x 520 with seed 2 does not (280 iterations against 440).  ``accepted`` / ``rejected`` count the trials."""

    def __init__(self, model: AdaptiveQuadModel, weights="next", **kw):
        super().__init__(model, **kw)
        assert weights in ("next", "used")
        self.weights = weights
        self.accepted = self.rejected = 0

    def objective_iterate(self, iters):
        for _ in range(int(iters)):
            self.k_adaptive += 1
            r = self.mo.rule(self.x, self.y, self.eta, self.omega, self.k_adaptive)
            self.xp, self.yp = self.x, self.y
            self.x, self.y, self.eta = r.x, r.y, r.eta_next
            w = r.eta_next if self.weights == "next" else r.weight
            self.xs, self.ys, self.ws = self.xs + w * self.x, self.ys + w * self.y, self.ws + w
            self.since += 1
            self.accepted += r.accepted
            self.rejected += not r.accepted


def adaptive_model_of(qp, qu=None, matrix=True):
    return AdaptiveQuadModel(qp.A, qp.m_ineq, qp.c, qp.q, qp.l, qp.u, qp.Q if matrix else None, qp.d, qu)
