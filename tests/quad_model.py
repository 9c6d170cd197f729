"""The diagonal quadratic objective ``c'x + 1/2 sum_j d_j x_j^2`` in float64 numpy with dense products: the model the tests of
tests/test_quad_host.py and tests/test_gpu_quad.py compare against (tests/ranged_model.py extended by ``d``: the oracle knows the
linear objective only), a numpy engine over it that ``run_pdlp`` can drive, and ``make_qp``, problems with a constructed optimum.
Needs no GPU."""
from types import SimpleNamespace

import numpy as np
import torch

from tests.ranged_model import RangedModel, RangedModelEngine
from torchpdlp_amd import _native as N


class QuadModel(RangedModel):
    """``RangedModel`` with the objective ``c'x + 1/2 sum_j d_j x_j^2``, ``d >= 0`` (None: zeros); ``qu``: two-sided rows as there"""

    def __init__(self, A, m_ineq, c, q, l, u, d=None, qu=None):
        super().__init__(A, m_ineq, c, q, l, u, qu)
        self.d = np.zeros(self.n) if d is None else np.asarray(d, np.float64).reshape(-1).copy()
        assert self.d.shape == (self.n,) and (self.d >= 0).all() and np.isfinite(self.d).all()

    # ---- the arithmetic of the issue -------------------------------------------------------------------------------------
    def step(self, x, y, tau, sigma, theta=1.0):
        """one PDHG step -> (x', y', xbar, K xbar): v = (x - tau (c - K'y)) / (1 + tau d), then the clamp"""
        xc = np.clip((x - tau * (self.c - self.A.T @ y)) / (1.0 + tau * self.d), self.l, self.u)
        xbar = xc + theta * (xc - x)
        k = self.A @ xbar
        return xc, self.dual(y, k, sigma), xbar, k

    # (halpern_step and adaptive_step of RangedModel go through step(): the combination and the step-size rule do not change)

    def half(self, x):
        """h = 1/2 sum_j d_j x_j^2 (invariant under the column scaling when d is scaled by D_col^2)"""
        return 0.5 * float(np.sum(self.d * x * x))

    def sums(self, x, y, d_col=None, d_row=None):
        """(the six raw sums in the library's slots, lam): [dual_res^2, l'lam+ - h, u'lam-, c'x + h, primal_res^2, q'y], and the
        reduced costs lam = project_lambda_box(c + D x - K'y); ``d_col`` / ``d_row``: of the un-scaled problem, the gradient formed
        BEFORE the division"""
        g, k = self.c + self.d * x - self.A.T @ y, self.A @ x
        h = self.half(x)
        c, l, u, q, qu = self.c, self.l, self.u, self.q, self.qu
        if d_col is not None:
            g, c, l, u, x = g / d_col, c / d_col, l * d_col, u * d_col, x * d_col
            k, q, qu, y = k / d_row, q / d_row, qu / d_row, y * d_row
        ninf, pinf = np.isneginf(l), np.isposinf(u)
        lam = np.where(ninf & pinf, 0.0, np.where(ninf, np.minimum(g, 0), np.where(pinf, np.maximum(g, 0), g)))
        lower = np.where(self.ineq, np.minimum(k - q, 0), k - q)
        with np.errstate(invalid="ignore"):
            upper = np.where(self.ineq & np.isfinite(qu), np.maximum(k - qu, 0), 0.0)
        side = np.where(self.ineq & (y < 0) & np.isfinite(qu), qu, q)
        s = np.array([np.sum((g - lam) ** 2), np.where(ninf, 0.0, l) @ np.maximum(lam, 0) - h, np.where(pinf, 0.0, u) @ np.minimum(lam, 0),
                      c @ x + h, np.sum(lower ** 2) + np.sum(upper ** 2), side @ y])
        return s, lam

    def kkt(self, x, y, omega, d_col=None, d_row=None):
        """the six numbers of PdlpEngine.kkt from the six sums, as rules.kkt_from_sums / pdlp_kkt_finish form them"""
        s, _ = self.sums(x, y, d_col, d_row)
        pr, dr, p, d_adj = np.sqrt(s[4]), np.sqrt(s[0]), s[3], s[5] + s[1] + s[2]
        gap = d_adj - p
        return dict(pr=pr, dr=dr, gap=gap, p=p, d_adj=d_adj, kkt=np.sqrt(omega ** 2 * pr ** 2 + dr ** 2 / omega ** 2 + gap ** 2))

    def objective(self, x):
        return float(self.c @ x) + self.half(x)


class QuadModelEngine(RangedModelEngine):
    """``RangedModelEngine`` over a ``QuadModel``, with the adaptive step as well: what solver.py uses of PdlpEngine.  ``quad``:
    whether the engine says it has the term (``quad_diag``), which is all the driver reads of it"""

    def __init__(self, model: QuadModel, quad=True, q_upper=False):
        super().__init__(model, q_upper=q_upper)
        self.quad_diag = torch.from_numpy(model.d.copy()) if quad else None
        self.delta = False
        self.k_adaptive = 0

    def set_step(self, eta, omega, theta=1.0, iteration=0):
        super().set_step(eta, omega, theta, iteration)
        self.k_adaptive = int(iteration)

    def iterate(self, iters, adaptive):
        if not adaptive:
            return super().iterate(iters, False)
        for _ in range(int(iters)):
            self.k_adaptive += 1
            self.xp, self.yp = self.x, self.y
            self.x, self.y, self.eta = self.mo.adaptive_step(self.x, self.y, self.eta, self.omega, self.k_adaptive)
            # (pdhg.py:107-108: an iterate is weighed with the step size the rule left behind)
            self.xs, self.ys, self.ws = self.xs + self.eta * self.x, self.ys + self.eta * self.y, self.ws + self.eta
            self.since += 1


def make_qp(m, n, seed, per_row=None, frac_ineq=0.6):
    """A QP ``min c'x + 1/2 x'Dx, K[:m_ineq] x >= q, K[m_ineq:] x = q, l <= x <= u`` with a constructed optimum, every number a
    small dyadic rational (so float32, float64 and the model see the same problem): x* with every bound class (free, lower only,
    upper only, boxed; on a bound or strictly inside), lam* consistent with x* (>= 0 on a lower bound, <= 0 on an upper bound, 0
    inside), y* (>= 0 on the active inequality rows, 0 on the inactive ones, either sign on the equality rows), d with about 40 %
    zeros, c = K'y* + lam* - d x*, q = K x* minus a slack on the inactive rows, opt = c'x* + 1/2 x*'Dx*.  ``per_row``: that many
    entries per row at random columns (default: dense with about half the entries).
    -> namespace(A scipy csr, m_ineq, c, q, l, u, d, opt, xs, ys, lam), float64 arrays"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    if per_row is None:
        Ad = rng.integers(-4, 5, size=(m, n)) / 2.0 * (rng.random((m, n)) < 0.5)
        A = sp.csr_matrix(Ad)
    else:
        rows, cols = np.repeat(np.arange(m), per_row), rng.integers(0, n, size=m * per_row)
        A = sp.coo_matrix((rng.integers(-4, 5, size=m * per_row) / 2.0, (rows, cols)), shape=(m, n)).tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    j = np.arange(n)
    kind = j % 4                                    # 0 free, 1 lower only, 2 upper only, 3 boxed
    l = np.where((kind == 1) | (kind == 3), -1.0, -np.inf)
    u = np.where((kind == 2) | (kind == 3), 2.0, np.inf)
    xs = rng.integers(-3, 8, n) / 4.0               # strictly inside (-1, 2)
    where = rng.integers(0, 3, n)                   # 0: inside, 1: on the lower bound, 2: on the upper bound (if it has that bound)
    at_l, at_u = (where == 1) & np.isfinite(l), (where == 2) & np.isfinite(u)
    xs[at_l], xs[at_u] = l[at_l], u[at_u]
    lam = np.zeros(n)
    lam[at_l] = rng.integers(1, 5, int(at_l.sum())) / 2.0
    lam[at_u] = -rng.integers(1, 5, int(at_u.sum())) / 2.0
    m_ineq = int(frac_ineq * m)
    i = np.arange(m)
    ineq = i < m_ineq
    active = ineq & (i % 2 == 0)
    ys = rng.integers(-4, 5, m) / 2.0
    ys[active] = np.abs(ys[active]) + 0.5
    ys[ineq & ~active] = 0.0
    d = rng.integers(1, 9, n) / 4.0 * (rng.random(n) >= 0.4)
    q = A @ xs
    q[ineq & ~active] -= rng.integers(1, 5, int((ineq & ~active).sum())) / 2.0
    c = A.T @ ys + lam - d * xs
    opt = float(c @ xs + 0.5 * np.sum(d * xs * xs))
    return SimpleNamespace(A=A, m=m, n=n, m_ineq=m_ineq, c=c, q=q, l=l, u=u, d=d, opt=opt, xs=xs, ys=ys, lam=lam)


def model_of_qp(qp, qu=None, quad=True):
    return QuadModel(qp.A, qp.m_ineq, qp.c, qp.q, qp.l, qp.u, qp.d if quad else None, qu)
