"""A plain numpy / scipy model of the population kernels (``pdlp_kernel_mv.inc``: k_csr_mv with the PrimalMV, DualMV, StoreMV and
GapMV epilogues, k_mv_dot, k_mv_finalize, k_mv_combine) and of their launchers (``pdlp_population.inc``: mv_steps_n, mv_gap_n,
mv_product_n), for an ``LP`` of ``tests/test_gpu_batch_kernels.py`` with shared vectors and populations ``X [n, j]``, ``Y [m, j]``.

Every function returns its value and, when the unit ``u`` of the kernel's working precision is given, an entrywise running-error
bound of the kernel's arithmetic by the rules at the top of ``tests/test_gpu_batch_kernels.py``: a row of length L may be off by
``(L + 1) u sum |K_ij| |v_j|`` plus the inputs' errors carried through ``|K|``; every further rounding adds u times the size of its
operands; the double sums add ``(len + 2) u64`` times the sum of their terms' sizes; the casts of mv_gap_n to T add u times each of
the four sums.  Every operation is continuous (the clamp, ``max(., 0)``, the projected lam), so the bounds carry through; where a
clamp or a projection holds with ``C_BOUND`` bounds to spare the result is the bound itself and exact.

``arith`` is the precision the values are computed in: float64 for the judge of ``tests/test_gpu_population_kernels.py``; the
working precision, optionally with every row's items in reverse order (``reverse=True``), for ``tests/test_population_model_host.py``,
which pins the model to the oracle and to the reference's recorded fishnet round first.
"""
import numpy as np
import scipy.sparse as sp

from tests.test_gpu_batch_kernels import C_BOUND, U64, gam


def _reversed(M):
    """M with the rows in reverse order and every row's items in reverse order (scipy adds a row's items as they are stored)"""
    nnz = M.indptr[-1]
    return sp.csr_matrix((M.data[::-1].copy(), M.indices[::-1].copy(), (nnz - M.indptr[::-1]).copy()), shape=M.shape)


class Arith:
    """the LP's data in the precision ``arith``: K and K' (items reversed if asked), c, q, l, u as columns"""

    def __init__(self, P, arith=np.float64, reverse=False):
        self.t, self.reverse = arith, reverse
        self.K, self.KT = (_reversed(M.astype(arith)) if reverse else M.astype(arith) for M in (P.K, P.KT))
        self.c, self.q, self.l, self.u = (v.astype(arith)[:, None] for v in P.col(0))

    def mul(self, M, V):
        V = np.ascontiguousarray(V, self.t)
        return (M @ V)[::-1] if self.reverse else M @ V


def _f64(*vs):
    return [np.asarray(v, np.float64) for v in vs]


def draw_population(P, j, rng):
    """X [n, j] as ``random_state`` draws x, clipped into the bounds in the even columns and left outside them in the odd ones;
    Y [m, j] with both signs on the inequality rows, so that the projection acts.  Values of the LP's precision, as float64."""
    _, _, l, u = P.col(0)
    X = rng.uniform(-1.5, 1.5, (P.n, j))
    X[:, 0::2] = np.clip(X[:, 0::2], l[:, None], u[:, None])
    Y = rng.uniform(-1, 1, (P.m, j))
    return X.astype(P.T).astype(np.float64), Y.astype(P.T).astype(np.float64)


def step_sizes(eta, omega, T):
    """tau and sigma as mv_steps_n rounds them: T(eta), T(omega), then T(e / w) and T(e * w)"""
    e, w = T(eta), T(omega)
    return T(e / w), T(e * w)


def product(P, X, u=None, arith=np.float64, reverse=False):
    """K X (StoreMV) -> value [m, j], bound"""
    A = Arith(P, arith, reverse)
    kx = A.mul(A.K, X)
    if u is None:
        return kx, None
    return kx, gam(P.Lr, u)[:, None] * (P.Ka @ np.abs(_f64(X)[0]))


def steps(P, X, Y, k, eta, omega, theta, T, u=None, arith=np.float64, reverse=False):
    """k PDHG_steps per column (PrimalMV then DualMV, k times) -> X, Y, bound of X, bound of Y (None without u)"""
    A = Arith(P, arith, reverse)
    t = arith
    tau, sigma = (t(v) for v in step_sizes(eta, omega, T))
    th = t(T(theta))
    x, y = np.array(X, t), np.array(Y, t)
    ex, ey = np.zeros(x.shape), np.zeros(y.shape)
    ineq = (np.arange(P.m) < P.m_ineq)[:, None]
    c, q, lo, hi = _f64(A.c, A.q, A.l, A.u)
    for _ in range(int(k)):
        # primal half: x+ = clamp(x - tau (c - K'y), l, u), xbar = x+ + theta (x+ - x)
        kty = A.mul(A.KT, y)
        g = A.c - kty
        p = tau * g
        v = x - p
        xn = np.minimum(np.maximum(v, A.l), A.u)
        d = xn - x
        xbar = xn + th * d
        if u is not None:
            e_g = P.KTa @ ey + gam(P.Lc, u)[:, None] * (P.KTa @ np.abs(_f64(y)[0])) + u * (np.abs(c) + np.abs(_f64(kty)[0]))
            e_p = float(tau) * e_g + u * np.abs(_f64(p)[0])
            e_v = ex + e_p + u * (np.abs(_f64(x)[0]) + np.abs(_f64(p)[0]))
            v64 = _f64(v)[0]
            clamped = (v64 + C_BOUND * e_v < lo) | (v64 - C_BOUND * e_v > hi)         # projected with room to spare: exact
            e_xn = np.where(clamped, 0.0, e_v)
            a_th = abs(float(th))
            e_xbar = e_xn + a_th * (e_xn + ex) + u * (2 * a_th * np.abs(_f64(d)[0]) + np.abs(_f64(xbar)[0]))
        # dual half: y+ = y + sigma (q - K xbar), the inequality rows projected onto y >= 0
        kx = A.mul(A.K, xbar)
        qk = A.q - kx
        sv = sigma * qk
        wv = y + sv
        yn = np.where(ineq & (wv < 0), t(0), wv)
        if u is not None:
            e_qk = P.Ka @ e_xbar + gam(P.Lr, u)[:, None] * (P.Ka @ np.abs(_f64(xbar)[0])) + u * (np.abs(q) + np.abs(_f64(kx)[0]))
            e_s = float(sigma) * e_qk + u * np.abs(_f64(sv)[0])
            e_w = ey + e_s + u * (np.abs(_f64(y)[0]) + np.abs(_f64(sv)[0]))
            ey = np.where(ineq & (_f64(wv)[0] + C_BOUND * e_w < 0), 0.0, e_w)
            ex = e_xn
        x, y = xn, yn
    return (x, y, ex, ey) if u is not None else (x, y, None, None)


def gap_terms(P, X, Y, u=None, arith=np.float64, reverse=False):
    """the four sums per column of mv_gap_n (GapMV: c'x, l_f'max(lam, 0), u_f'min(lam, 0) with lam = project_lambda_box(c - K'y);
    k_mv_dot: q'y), added in double -> S [4, j], bound [4, j], the sums of the terms' sizes [4, j]"""
    A = Arith(P, arith, reverse)
    t = arith
    x, y = np.asarray(X, t), np.asarray(Y, t)
    kty = A.mul(A.KT, y)
    g = A.c - kty
    ninf, pinf = np.isneginf(A.l), np.isposinf(A.u)
    zero = t(0)
    lam = np.where(ninf & pinf, zero, np.where(ninf, np.minimum(g, zero), np.where(pinf, np.maximum(g, zero), g)))
    ld, ud = np.where(ninf, zero, A.l), np.where(pinf, zero, A.u)
    lp, ln = np.maximum(lam, zero), np.minimum(lam, zero)
    d = lambda a, b: _f64(a)[0] * _f64(b)[0]
    terms = [d(A.c, x), d(ld, lp), d(ud, ln), d(A.q, y)]
    if reverse:
        terms = [tm[::-1] for tm in terms]
    S = np.stack([tm.sum(0) for tm in terms])
    sizes = np.stack([np.abs(tm).sum(0) for tm in terms])
    if u is None:
        return S, None, sizes
    e_g = gam(P.Lc, u)[:, None] * (P.KTa @ np.abs(_f64(y)[0])) + u * (np.abs(_f64(A.c)[0]) + np.abs(_f64(kty)[0]))
    e_lam = np.where(ninf & pinf, 0.0, e_g)
    errs = [0.0 * terms[0], np.abs(_f64(ld)[0]) * e_lam, np.abs(_f64(ud)[0]) * e_lam, 0.0 * terms[3]]
    E = np.stack([e.sum(0) + (tm.shape[0] + 2) * U64 * np.abs(tm).sum(0) for tm, e in zip(terms, errs)])
    return S, E, sizes


def gap_from_terms(S, T, E=None, u=None):
    """the gap of every column from the four double sums in the working precision, as mv_gap_n: each sum cast to T,
    ``adj = q'y + l_f'lam+ + u_f'lam-``, ``gap = adj - c'x`` -> gap [j] (float64 of the T value), bound"""
    p, lp, un, d = (np.asarray(s, np.float64).astype(T) for s in S)
    first = d + lp
    adj = first + un
    gap = adj - p
    if E is None:
        return gap.astype(np.float64), None
    a = lambda v: np.abs(np.asarray(v, np.float64))
    e = E.sum(0) + u * a(S).sum(0) + u * (a(first) + a(adj) + a(gap))
    return gap.astype(np.float64), e


def gap(P, X, Y, T, u=None, arith=np.float64, reverse=False):
    S, E, _ = gap_terms(P, X, Y, u, arith, reverse)
    return gap_from_terms(S, T, E, u)


def combine(V, W, u=None, arith=np.float64, reverse=False):
    """V W (k_mv_combine: p in order) -> value [rows, nw], bound"""
    v, w = np.asarray(V, arith), np.asarray(W, arith)
    out = np.zeros((v.shape[0], w.shape[1]), arith)
    order = range(v.shape[1])
    for p in (reversed(order) if reverse else order):
        out = out + v[:, p:p + 1] * w[p:p + 1, :]
    if u is None:
        return out, None
    return out, gam(v.shape[1], u) * (np.abs(_f64(v)[0]) @ np.abs(_f64(w)[0]))
