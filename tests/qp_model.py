"""The sparse quadratic objective ``c'x + 1/2 x'Qx`` in float64 numpy with dense products: ``QuadModel`` (tests/quad_model.py) extended
by a dense symmetric ``Q`` and the linearised step, the model the tests of tests/test_quad_matrix_host.py and
tests/test_gpu_quad_matrix.py compare against; a numpy engine over it that ``run_pdlp`` can drive; and ``make_general_qp``, problems
with a constructed optimum.  Needs no GPU."""
import numpy as np
import torch

from tests.quad_model import QuadModel, QuadModelEngine, make_qp


class GeneralQuadModel(QuadModel):
    """``QuadModel`` with the objective ``c'x + 1/2 x'Qx + 1/2 sum_j d_j x_j^2``: ``Q`` dense (or scipy sparse), symmetric (None: zeros)"""

    def __init__(self, A, m_ineq, c, q, l, u, Q=None, d=None, qu=None):
        super().__init__(A, m_ineq, c, q, l, u, d, qu)
        Q = np.zeros((self.n, self.n)) if Q is None else Q
        self.Q = np.asarray(Q.todense() if hasattr(Q, "todense") else Q, np.float64)
        assert self.Q.shape == (self.n, self.n) and np.array_equal(self.Q, self.Q.T)

    # ---- the arithmetic of the issue -------------------------------------------------------------------------------------
    def grad(self, x):
        """g = c + Q x: what the primal half-step and the KKT pass read where they read c"""
        return self.c + self.Q @ x

    def step(self, x, y, tau, sigma, theta=1.0):
        """one linearised PDHG step -> (x', y', xbar, K xbar): x' = clamp((x - tau (g - K'y)) / (1 + tau d), l, u) with g = c + Q x"""
        xc = np.clip((x - tau * (self.grad(x) - self.A.T @ y)) / (1.0 + tau * self.d), self.l, self.u)
        xbar = xc + theta * (xc - x)
        k = self.A @ xbar
        return xc, self.dual(y, k, sigma), xbar, k

    def half(self, x):
        """h = 1/2 x'Qx + 1/2 sum_j d_j x_j^2 (invariant under the column scaling with D_col Q D_col and d D_col^2)"""
        return 0.5 * float(x @ (self.Q @ x)) + super().half(x)

    def sums(self, x, y, d_col=None, d_row=None):
        """(the six raw sums in the library's slots, lam): [dual_res^2, l'lam+ - h, u'lam-, c'x + h, primal_res^2, q'y] with the
        reduced costs lam = project_lambda_box(c + Q x + D x - K'y); ``d_col`` / ``d_row``: of the un-scaled problem, the gradient
        formed BEFORE the division"""
        g, k = self.grad(x) + self.d * x - self.A.T @ y, self.A @ x
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

    # (kkt of QuadModel goes through sums(); objective through half())


class GeneralQuadEngine(QuadModelEngine):
    """``QuadModelEngine`` over a ``GeneralQuadModel``: what solver.py uses of PdlpEngine for the fixed, linearised step.  ``steps``
    records every ``(eta, omega, iteration)`` the driver sets and ``omegas`` every primal weight it sets alone; ``scaling`` =
    ``(D_col, D_row)``: the model is a scaled problem, and ``kkt(unscaled=True)`` gives the numbers of the original one"""

    def __init__(self, model: GeneralQuadModel, quad_diag=False, q_upper=False, scaling=None):
        super().__init__(model, quad=quad_diag, q_upper=q_upper)
        self.scaling = scaling
        self.quad_matrix = torch.from_numpy(model.Q.copy())
        self.steps, self.omegas = [], []

    def set_step(self, eta, omega, theta=1.0, iteration=0):
        super().set_step(eta, omega, theta, iteration)
        self.steps.append((float(eta), float(omega), int(iteration)))

    def set_omega(self, omega):
        super().set_omega(omega)
        self.omegas.append(float(omega))

    def iterate(self, iters, adaptive):
        assert not adaptive
        return super().iterate(iters, False)

    def kkt(self, which, omega, unscaled=False):
        dd = self.scaling if unscaled else (None, None)
        return {k: float(v) for k, v in self.mo.kkt(*self._point(which), float(omega), *dd).items()}

    def halpern_iterate(self, iters):
        raise AssertionError("no Halpern iteration with a sparse quadratic objective")

    def objective_product(self, v):
        return torch.from_numpy(self.mo.Q @ v.numpy().astype(np.float64))

    def power_iteration(self, b0, iters=100):
        b = b0.numpy().astype(np.float64)
        for _ in range(int(iters)):
            b = self.mo.A.T @ (self.mo.A @ b)
            b /= np.linalg.norm(b)
        return float(np.linalg.norm(self.mo.A @ b))


KINDS = ("lowrank", "sparse", "arrow")


def quad_matrix_of(n, seed, kind):
    """the three matrices of the issue as scipy csr, every entry a small dyadic rational; ``rng = default_rng(1000 + seed)``:
    "lowrank" F'F with F 6 x n, entries integers(-2, 3) / 2 kept with probability 0.3; "sparse" B'B with B n x n, per row one entry
    integers(1, 4) / 2 and one entry integers(-3, 0) / 2 at random columns, 30 % of the rows zeroed; "arrow" the identity plus 2^-6
    along row and column 0 (row 0 is longer than the CSR kernel's block once n > 2048)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(1000 + seed)
    if kind == "lowrank":
        F = rng.integers(-2, 3, size=(6, n)) / 2.0 * (rng.random((6, n)) < 0.3)
        Q = sp.csr_matrix(F.T @ F)
    elif kind == "sparse":
        r = np.arange(n)
        B = sp.coo_matrix((rng.integers(1, 4, n) / 2.0, (r, rng.integers(0, n, n))), shape=(n, n)).tocsr()
        B = B + sp.coo_matrix((rng.integers(-3, 0, n) / 2.0, (r, rng.integers(0, n, n))), shape=(n, n)).tocsr()
        B = sp.diags((rng.random(n) >= 0.3).astype(np.float64)) @ B
        Q = (B.T @ B).tocsr()
    elif kind == "arrow":
        Q = sp.identity(n, format="lil")
        Q[0, 1:] = 2.0 ** -6
        Q[1:, 0] = 2.0 ** -6
        Q = Q.tocsr()
    else:
        raise ValueError(kind)
    Q.eliminate_zeros()
    Q.sort_indices()
    assert (abs(Q - Q.T)).nnz == 0
    return Q


def make_general_qp(m, n, seed, per_row=None, kind="lowrank", diag=False):
    """``make_qp``'s instance with the objective ``c'x + 1/2 x'Qx`` (``diag``: ``+ 1/2 x'Dx`` with ``make_qp``'s ``d`` as well, else
    ``d = 0``): the same K, q, l, u, x*, y*, lam*, and ``c = K'y* + lam* - Q x* - d x*`` with ``opt`` to match, so x* stays optimal.
    -> ``make_qp``'s namespace with ``Q`` (scipy csr) added"""
    qp = make_qp(m, n, seed, per_row=per_row)
    Q = quad_matrix_of(n, seed, kind)
    if not diag:
        qp.c = qp.c + qp.d * qp.xs
        qp.d = np.zeros(n)
    qp.c = qp.c - Q @ qp.xs
    qp.Q = Q
    qp.opt = float(qp.c @ qp.xs + 0.5 * np.sum(qp.d * qp.xs * qp.xs) + 0.5 * qp.xs @ (Q @ qp.xs))
    return qp


def model_of_general_qp(qp, qu=None, matrix=True):
    return GeneralQuadModel(qp.A, qp.m_ineq, qp.c, qp.q, qp.l, qp.u, qp.Q if matrix else None, qp.d, qu)
