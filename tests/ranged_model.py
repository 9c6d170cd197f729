"""Two-sided rows ``q <= K x <= q_upper`` in float64 numpy with dense products: the model the tests of tests/test_ranged_rows_host.py
and tests/test_gpu_ranged_rows.py compare against (the oracle knows one-sided rows only), and a numpy engine over it that
``run_pdlp`` can drive, in the style of tests/test_halpern_host.py:HalpernOracleEngine.  Needs no GPU."""
import numpy as np
import torch

from torchpdlp_amd import _native as N


class RangedModel:
    """``A`` dense (m, n); rows ``i < m_ineq``: ``q_i <= (A x)_i <= qu_i`` (``qu_i = +inf``: one-sided), the others ``(A x)_i = q_i``"""

    def __init__(self, A, m_ineq, c, q, l, u, qu=None):
        self.A = np.asarray(A.todense() if hasattr(A, "todense") else A, np.float64)
        self.m, self.n = self.A.shape
        self.m_ineq = int(m_ineq)
        self.c, self.q, self.l, self.u = (np.asarray(v, np.float64).reshape(-1) for v in (c, q, l, u))
        self.qu = np.full(self.m, np.inf) if qu is None else np.asarray(qu, np.float64).reshape(-1).copy()
        self.qu[self.m_ineq:] = np.inf                     # (ignored on the equality rows)
        self.ineq = np.arange(self.m) < self.m_ineq

    # ---- the arithmetic of the issue -------------------------------------------------------------------------------------
    def dual(self, y, k, sigma):
        """y' from k = (A xbar): a = y + sigma (q - k), b = y + sigma (qu - k); a > 0 ? a : (b < 0 ? b : 0) on the inequality rows"""
        a = y + sigma * (self.q - k)
        with np.errstate(invalid="ignore"):
            b = y + sigma * (self.qu - k)
        return np.where(self.ineq, np.where(a > 0, a, np.where(b < 0, b, 0.0)), a)

    def sides(self, y, k, sigma):
        """(lower active, upper active, neither) on the rows that have both sides and a gap between them"""
        a = y + sigma * (self.q - k)
        with np.errstate(invalid="ignore"):
            b = y + sigma * (self.qu - k)
        two = self.ineq & np.isfinite(self.qu) & (self.qu > self.q)
        return two & (a > 0), two & (b < 0), two & ~(a > 0) & ~(b < 0)

    def step(self, x, y, tau, sigma, theta=1.0):
        """one PDHG step -> (x', y', xbar, K xbar)"""
        xc = np.clip(x - tau * (self.c - self.A.T @ y), self.l, self.u)
        xbar = xc + theta * (xc - x)
        k = self.A @ xbar
        return xc, self.dual(y, k, sigma), xbar, k

    def halpern_step(self, x, y, xa, ya, t, tau, sigma):
        """tests/test_gpu_halpern.py:model_step with the two-sided dual step -> (x+, y+, x', y')"""
        a, b = (t + 1) / (t + 2), 1 / (t + 2)
        xc, yc, xbar, _ = self.step(x, y, tau, sigma)
        return a * xbar + b * xa, a * (2 * yc - y) + b * ya, xc, yc

    def adaptive_step(self, x, y, eta, omega, k):
        """oracle/torch_coo.py:step_adaptive (one trial, kept even when rejected) with the two-sided dual step -> (x', y', eta')"""
        xc, yc, _, _ = self.step(x, y, eta / omega, eta * omega)
        dx, dy = xc - x, yc - y
        den = 2 * (dy @ (self.A @ dx))
        if den != 0:
            eta_bar = (omega * (dx @ dx) + (dy @ dy) / omega) / abs(den)
            t1 = (1 - (k + 1) ** (-0.3)) * eta_bar
        else:
            eta_bar = t1 = np.inf
        return xc, yc, min(t1, (1 + (k + 1) ** (-0.6)) * eta)

    def kkt(self, x, y, omega, d_col=None, d_row=None):
        """the six numbers of PdlpEngine.kkt; ``d_col`` / ``d_row``: of the un-scaled problem (x_u = D_col x, y_u = D_row y, ...)"""
        g, k = self.c - self.A.T @ y, self.A @ x
        c, l, u, q, qu = self.c, self.l, self.u, self.q, self.qu
        if d_col is not None:
            g, c, l, u, x = g / d_col, c / d_col, l * d_col, u * d_col, x * d_col
            k, q, qu, y = k / d_row, q / d_row, qu / d_row, y * d_row
        ninf, pinf = np.isneginf(l), np.isposinf(u)
        lam = np.where(ninf & pinf, 0.0, np.where(ninf, np.minimum(g, 0), np.where(pinf, np.maximum(g, 0), g)))
        lower = np.where(self.ineq, np.minimum(k - q, 0), k - q)
        upper = np.where(self.ineq, np.maximum(k - qu, 0), 0.0)
        pr, dr = np.sqrt(np.sum(lower ** 2) + np.sum(upper ** 2)), np.linalg.norm(g - lam)
        side = np.where(self.ineq & (y < 0) & np.isfinite(qu), qu, q)
        d_adj = side @ y + np.where(ninf, 0.0, l) @ np.maximum(lam, 0) + np.where(pinf, 0.0, u) @ np.minimum(lam, 0)
        p = c @ x
        gap = d_adj - p
        return dict(pr=pr, dr=dr, gap=gap, p=p, d_adj=d_adj, kkt=np.sqrt(omega ** 2 * pr ** 2 + dr ** 2 / omega ** 2 + gap ** 2))

    def norm_q(self):
        """the norm that stands for ||q||: max(|q_i|, |qu_i|) on the two-sided rows"""
        two = self.ineq & np.isfinite(self.qu)
        return float(np.linalg.norm(np.where(two, np.maximum(np.abs(self.q), np.abs(self.qu)), self.q)))


class RangedModelEngine:
    """what solver.py uses of PdlpEngine for averaged fixed-step PDHG and for the Halpern mode, over a ``RangedModel`` in float64"""

    def __init__(self, model: RangedModel, q_upper=True):
        self.mo = model
        self.dtype, self.device, self.comm, self.mixed = torch.float64, torch.device("cpu"), None, False
        self.n, self.m, self.nl, self.ml, self.m_ineq = model.n, model.m, model.n, model.m, model.m_ineq
        self.q, self.c = torch.from_numpy(model.q.copy()), torch.from_numpy(model.c.copy())
        self.q_upper = torch.from_numpy(model.qu.copy()) if q_upper else None

    def set_iterate(self, x, y):
        self.x, self.y = x.numpy().astype(np.float64).copy(), y.numpy().astype(np.float64).copy()
        self.xp, self.yp = self.x.copy(), self.y.copy()
        self.x_last, self.y_last = self.x.copy(), self.y.copy()
        self._reset()

    def _reset(self):
        self.xs, self.ys, self.ws, self.since = np.zeros(self.n), np.zeros(self.m), 0.0, 0
        self.xa = self.ya = None

    def set_step(self, eta, omega, theta=1.0, iteration=0):
        self.eta, self.omega = float(eta), float(omega)

    def set_omega(self, omega):
        self.omega = float(omega)

    def iterate(self, iters, adaptive):
        assert not adaptive
        for _ in range(int(iters)):
            self.xp, self.yp = self.x, self.y
            self.x, self.y, _, _ = self.mo.step(self.x, self.y, self.eta / self.omega, self.eta * self.omega)
            self.xs, self.ys, self.ws = self.xs + self.eta * self.x, self.ys + self.eta * self.y, self.ws + self.eta
            self.since += 1

    def halpern_iterate(self, iters):
        for _ in range(int(iters)):
            self.x, self.y, self.xa, self.ya = self.mo.halpern_step(self.x, self.y, self.x_last, self.y_last, self.since,
                                                                    self.eta / self.omega, self.eta * self.omega)
            self.since += 1

    def flush_average(self, adaptive=True):
        pass

    def compute_average(self):
        self.xa, self.ya = self.xs / self.ws, self.ys / self.ws

    def _point(self, which):
        return {N.CUR: (self.x, self.y), N.AVG: (self.xa, self.ya), N.PREV: (self.xp, self.yp)}[which]

    def kkt(self, which, omega, unscaled=False):
        return {k: float(v) for k, v in self.mo.kkt(*self._point(which), float(omega)).items()}

    def restart(self, which):
        if which == N.AVG:
            self.x, self.y = self.xa, self.ya
        self._reset()

    def restart_distance(self):
        return float(np.sum((self.x_last - self.x) ** 2)), float(np.sum((self.y_last - self.y) ** 2))

    def mark_restart_point(self):
        self.x_last, self.y_last = self.x.copy(), self.y.copy()

    def get_iterate(self, which=N.CUR):
        x, y = self._point(which)
        return torch.from_numpy(x.copy()), torch.from_numpy(y.copy())

    def synchronize(self):
        pass


def split_model(mo: RangedModel) -> RangedModel:
    """the split twin: every two-sided row entered twice, one-sided rows only"""
    from torchpdlp_amd.ranged import split_rows
    import scipy.sparse as sp
    As, qs, mi, _ = split_rows(sp.csr_matrix(mo.A), mo.q, mo.qu, mo.m_ineq)
    return RangedModel(As, mi, mo.c, qs, mo.l, mo.u)


def feasible_ranged_lp(m, n, per_row, seed, frac_ineq=0.6):
    """A feasible, bounded two-sided LP whose numbers are float32 values: random sparse rows, a point x* inside a box, and row sides
    placed around A x*, an objective for which x* is optimal (so the LP is bounded): inequality rows cycle through (q, +inf), (q, q_upper) with x* strictly inside, (q, q_upper) with x* on the
    UPPER side, (q, q) -- so some upper sides are active at the optimum's neighbourhood -- then equality rows.
    -> (A scipy csr, m_ineq, c, q, l, u, q_upper), float64 arrays."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    rows, cols = np.repeat(np.arange(m), per_row), rng.integers(0, n, size=m * per_row)
    A = sp.coo_matrix((f32(rng.integers(-4, 5, size=m * per_row) / 2.0), (rows, cols)), shape=(m, n)).tocsr()
    A.sort_indices()
    xs = f32(rng.integers(0, 9, n) / 4.0)                               # in [0, 2], multiples of 1/4: A x* is exact
    k = A @ xs
    m_ineq = int(frac_ineq * m)
    q, qu = k.copy(), np.full(m, np.inf)
    kind = np.arange(m) % 4
    i = np.arange(m) < m_ineq
    q[i & (kind == 0)] -= 0.5
    q[i & (kind == 1)] -= 1.0
    qu[i & (kind == 1)] = k[i & (kind == 1)] + 0.75
    q[i & (kind == 2)] -= 1.5
    qu[i & (kind == 2)] = k[i & (kind == 2)]
    qu[i & (kind == 3)] = q[i & (kind == 3)]
    # an objective for which x* is optimal: c = A'y* + lam with y* < 0 where x* sits on an upper side, 0 where it is strictly inside,
    # of either sign on the (q, q) and the equality rows, and reduced costs lam >= 0 on the variables at their lower bound 0
    ys = f32(rng.integers(-4, 5, m) / 2.0)
    ys[i & (kind <= 1)] = 0.0
    ys[i & (kind == 2)] = -np.abs(ys[i & (kind == 2)]) - 0.5
    c = f32(A.T @ ys + np.where(xs == 0, rng.integers(1, 4, n) / 2.0, 0.0))
    u = np.full(n, 3.0)
    u[::3] = np.inf                                                      # (a third of the variables without an upper bound)
    return A, m_ineq, c, f32(q), np.zeros(n), u, f32(qu)
