"""The batched kernels (pdlp_batch_*) one call at a time against a float64 reference of the same operation on the same inputs.

Every test drives ``BatchEngine`` directly: it writes the populations and per-LP scalars, calls ``iterate``, ``average``, ``kkt`` or
``restart`` once, reads everything back and compares every live column with

- ``oracle.OracleLP(..., dtype=np.float64)`` for what the oracle has (the fixed and the adaptive step, the KKT residuals, whole solves),
- a few lines of float64 numpy below for the rest (the weighted sums, ``eta_sum``, ``wpend``, the average, the restart bookkeeping and
  the squared restart distances, the six raw KKT sums).

Tolerances are running-error bounds of the kernel's own arithmetic, carried through the operation entry by entry: a product
``sum_j K_ij v_j`` of a row of length L may be off by ``(L + 1) u sum_j |K_ij| |v_j|`` (u: the unit of the working precision) plus
what the inputs' errors carry through ``|K|``; every other rounding adds ``u`` times the size of its operands; the double sums add
``(len + 2) u64`` times the sum of their terms' sizes.  The comparison allows ``C_BOUND`` times that bound: a factor 2 for the
reference's own roundings and 2 for second-order terms.  In float64 this is far below a relative 1e-12.

Columns that are frozen (``live == 0``) or padding hold a signalling-NaN bit pattern in every population, in the per-LP vectors and in
the per-LP scalars; every call must leave those bytes as they were (compared through an integer view) and every live column must come
out finite and match the reference.
"""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import torchpdlp_amd as tp
from torchpdlp_amd import _native as N
from torchpdlp_amd.batch import BatchEngine, group_width, pdlp_algorithm_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
C_BOUND = 4.0
U64 = np.finfo(np.float64).eps
POISON = {np.float32: (np.uint32, 0x7FA5A5A5), np.float64: (np.uint64, 0x7FF4A5A5A5A5A5A5)}   # signalling NaNs with a payload
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
IVIEW = {torch.float32: torch.int32, torch.float64: torch.int64, torch.int32: torch.int32}
XPOP = ("x", "x_prev", "xbar", "x_sum", "x_avg", "x_last")
YPOP = ("y", "y_prev", "y_sum", "y_avg", "y_last", "dy")
SCAL = ("eta", "omega", "eta_sum", "wpend")


def dev():
    return torch.device("cuda", 0)


def poison(shape, T):
    it, bits = POISON[T]
    return np.full(shape, bits, dtype=it).view(T)


# ---------------------------------------------------------------------------------------------------------------------------------
# the LPs
# ---------------------------------------------------------------------------------------------------------------------------------
class LP:
    """K (CSR, values already in the working precision T) and c, q, l, u, each shared (1-D) or per LP ([len, B])"""

    def __init__(self, m, n, m_ineq, rp, ci, va, c, q, l, u, T):
        self.m, self.n, self.m_ineq, self.T = int(m), int(n), int(m_ineq), T
        self.rp, self.ci = np.asarray(rp, np.int64), np.asarray(ci, np.int32)
        self.va = np.asarray(va, T)
        # CSR as given (a row may hold a column twice: the kernels add both items); scipy never gets to merge them in place
        mk = lambda v: sp.csr_matrix((v, self.ci.copy(), self.rp.copy()), shape=(self.m, self.n))
        self.K, self.Ka = mk(self.va.astype(np.float64)), mk(np.abs(self.va.astype(np.float64)))
        self.KT, self.KTa = self.K.T.tocsr(), self.Ka.T.tocsr()
        self.Lr = np.diff(self.rp).astype(np.float64)
        self.Lc = np.bincount(self.ci, minlength=self.n).astype(np.float64)
        Kt = mk(self.va.astype(np.float64)).T.tocsr()          # the oracle's own K' (oracle.OracleLP), built once
        Kt.sort_indices()
        self._trans = (Kt.indptr.astype(np.int32), Kt.indices.astype(np.int32), Kt.data)
        self.vec = [np.asarray(v, T) for v in (c, q, l, u)]

    def col(self, b):
        return [(v if v.ndim == 1 else v[:, b]).astype(np.float64) for v in self.vec]

    def oracle(self, b, K=None, vec=None):
        """the float64 oracle of column b (or of a given float64 matrix and vectors: the un-scaled LP)"""
        from oracle import oracle as orc
        if K is None:
            c, q, l, u = self.col(b)
            return orc.OracleLP(self.m, self.n, self.m_ineq, self.rp.astype(np.int32), self.ci, self.va.astype(np.float64), c, q, l, u,
                                dtype=np.float64, trans=self._trans)
        Kt = K.T.tocsr()
        Kt.sort_indices()
        return orc.OracleLP(self.m, self.n, self.m_ineq, K.indptr, K.indices, K.data, *vec, dtype=np.float64,
                            trans=(Kt.indptr, Kt.indices, Kt.data))

    def csr(self):
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dt)
        return tp.CsrPair(self.m, self.n, t(self.rp, torch.int64), t(self.ci, torch.int32), t(self.va, TORCH[self.T])).to(dev())


def csr_of_rows(m, n, rows, vals):
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.concatenate([np.sort(np.asarray(r, np.int64)) for r in rows]).astype(np.int32) if rp[-1] else np.zeros(0, np.int32)
    return rp, ci, np.asarray(vals[:rp[-1]])


def bounds_mix(n, rng, T, B=None):
    """l, u with every bound class of project_lambda_box: boxed, fixed, lower-only, upper-only, free (per column if B)"""
    shape = (n,) if B is None else (n, B)
    kind = rng.integers(0, 5, shape)
    lo = rng.uniform(-2, 0, shape)
    hi = lo + rng.uniform(0.5, 3, shape)
    l = np.where(kind == 3, -np.inf, np.where(kind == 4, -np.inf, lo))
    u = np.where(kind == 1, lo, np.where(kind == 2, np.inf, np.where(kind == 4, np.inf, hi)))
    return l.astype(T), u.astype(T)


def golden_lp(T, B, rng, per="CQLU", file="step_adaptive.npz", name="mixed_400x300"):
    """the golden 400 x 300 LP as column 0; the other columns perturb c and q and draw bounds of every class"""
    g = np.load(os.path.join(GOLDEN, file))
    a = lambda k: g[f"{name}/{k}"]
    m, n = int(a("m")), int(a("n"))
    c0, q0, l0, u0 = (a(k).astype(np.float64) for k in ("c", "q", "l", "u"))
    C = np.stack([c0] + [c0 * (1 + 0.3 * rng.standard_normal(n)) for _ in range(1, B)], 1)
    Q = np.stack([q0] + [q0 * (1 + 0.3 * rng.standard_normal(m)) + 0.1 * rng.standard_normal(m) for _ in range(1, B)], 1)
    Lb, Ub = bounds_mix(n, rng, np.float64, B)
    Lb[:, 0], Ub[:, 0] = l0, u0
    pick = lambda v, v0, flag: v if flag.isupper() else v0
    vec = [pick(v, v0, f) for v, v0, f in zip((C, Q, Lb, Ub), (c0, q0, l0, u0), per)]
    return LP(m, n, int(a("m_ineq")), a("rowptr"), a("colidx"), a("val"), *vec, T=T), g


def shape_lp(name, T, B, per, rng):
    """the edge shapes of the single-LP suite"""
    if name == "1x1":
        m, n, rows, mi = 1, 1, [[0]], 0
    elif name == "ineq0":
        m, n, mi = 23, 17, 0
        rows = [rng.choice(n, 3, replace=False) for _ in range(m)]
    elif name == "ineq_all":
        m, n = 19, 29
        mi = m
        rows = [rng.choice(n, 4, replace=False) for _ in range(m)]
    elif name == "empty_rows_cols":           # rows 0, 5, 11 and columns 0, 7, 13 hold nothing
        m, n, mi = 30, 20, 12
        live_cols = np.setdiff1d(np.arange(n), [0, 7, 13])
        rows = [[] if i in (0, 5, 11) else rng.choice(live_cols, 3, replace=False) for i in range(m)]
    elif name == "long_row":                  # a row of 150 items and a column of 140 (longer than a wave either way)
        m, n, mi = 140, 150, 70
        rows = [np.arange(n)] + [np.union1d([3], rng.choice(n, 2, replace=False)) for _ in range(m - 1)]
    elif name == "odd_rows":                  # not a multiple of 64 / W rows for any W
        m, n, mi = 37, 41, 20
        rows = [rng.choice(n, 1 + i % 5, replace=False) for i in range(m)]
    else:
        raise KeyError(name)
    rp, ci, _ = csr_of_rows(m, n, rows, np.zeros(0))
    va = rng.uniform(0.2, 2.0, ci.size) * rng.choice([-1, 1], ci.size)
    c = rng.standard_normal((n, B))
    q = rng.standard_normal((m, B))
    L, U = bounds_mix(n, rng, np.float64, B)
    shared = lambda v: v[:, 0]
    vec = [v if f.isupper() else shared(v) for v, f in zip((c, q, L, U), per)]
    return LP(m, n, mi, rp, ci, va, *vec, T=T)


def big_lp(T, B, rng, m=300_000, n=70_000):
    """3 items per row, past BATCH_MAXG workgroups for K at every W and for K' at W = 32; built as CSR"""
    i = np.arange(m, dtype=np.int64)
    ci = np.sort(np.stack([i % n, (i * 7 + 1) % n, (i * 13 + 5) % n], 1), axis=1)
    same = (ci[:, 1:] == ci[:, :-1]).any(1)
    ci[same] = np.sort(np.stack([i[same] % n, (i[same] + 1) % n, (i[same] + 2) % n], 1), axis=1)
    rp = np.arange(0, 3 * m + 1, 3, dtype=np.int64)
    va = rng.uniform(0.2, 1.0, 3 * m) * rng.choice([-1, 1], 3 * m)
    L, U = bounds_mix(n, rng, np.float64, B)
    return LP(m, n, m // 2, rp, ci.reshape(-1).astype(np.int32), va, rng.standard_normal((n, B)), rng.standard_normal(m), L, U, T=T)


def eta_base(P):
    """0.9 / ||K||_2 with ||K||_2 <= sqrt(||K||_1 ||K||_inf)"""
    n1 = max(float(P.Ka.sum(0).max()), 1e-30)
    ninf = max(float(P.Ka.sum(1).max()), 1e-30)
    return 0.9 / np.sqrt(n1 * ninf)


# ---------------------------------------------------------------------------------------------------------------------------------
# the batch under test
# ---------------------------------------------------------------------------------------------------------------------------------
def random_state(P, Bp, live_cols, rng, eta_spread):
    """populations and per-LP scalars: random in the live columns, the poison pattern everywhere else"""
    T = P.T
    st = {}
    for names, ln in ((XPOP, P.n), (YPOP, P.m)):
        for nm in names:
            st[nm] = poison((ln, Bp), T)
    nl = len(live_cols)
    for b in live_cols:
        c, q, l, u = P.col(b)
        x = np.clip(rng.uniform(-1.5, 1.5, P.n), l, u)
        st["x"][:, b] = x
        for nm in ("x_prev", "x_sum", "x_avg", "x_last", "xbar"):
            st[nm][:, b] = rng.uniform(-1, 1, P.n)
        y = rng.uniform(-1, 1, P.m)
        y[:P.m_ineq] = np.abs(y[:P.m_ineq])
        st["y"][:, b] = y
        for nm in ("y_prev", "y_sum", "y_avg", "y_last", "dy"):
            st[nm][:, b] = rng.uniform(-1, 1, P.m)
    e0 = eta_base(P)
    sc = {nm: poison(Bp, T) for nm in SCAL}
    sc["eta"][live_cols] = e0 * np.exp(rng.uniform(np.log(eta_spread[0]), np.log(eta_spread[1]), nl))
    sc["omega"][live_cols] = np.exp(rng.uniform(np.log(0.5), np.log(2.0), nl))
    sc["eta_sum"][live_cols] = rng.uniform(1.0, 3.0, nl) * e0 * 10
    sc["wpend"][live_cols] = rng.uniform(0.5, 1.5, nl) * e0
    st.update(sc)
    live = np.zeros(Bp, np.int32)
    live[live_cols] = 1
    st["live"], st["action"] = live, np.zeros(Bp, np.int32)
    return st


class Batch:
    """a BatchEngine with random live columns and poisoned frozen and padding columns; ``pull`` reads the live columns as float64"""

    def __init__(self, P, B, W=None, frozen=(), rng=None, D=None, eta_spread=(0.3, 3.0)):
        self.P, self.B, T = P, B, P.T
        self.dt = TORCH[T]
        d = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev())
        dcol, drow = (None, None) if D is None else (d(D[0].astype(T)), d(D[1].astype(T)))
        self.be = be = BatchEngine(P.csr(), P.m_ineq, *(d(v) for v in P.vec), B, d_col=dcol, d_row=drow, W=W)
        self.Bp = be.Bp
        self.live = np.array([b for b in range(B) if b not in set(frozen)])
        self.dead = np.setdiff1d(np.arange(self.Bp), self.live)
        rng = np.random.default_rng(0) if rng is None else rng
        st = random_state(P, self.Bp, self.live, rng, eta_spread)
        self.write(**st)
        for i, v in enumerate(be.vec):          # the per-LP vectors' frozen and padding columns
            if v.dim() == 2:
                v[:, self.dead] = torch.from_numpy(poison((v.shape[0], len(self.dead)), T)).to(dev())
        torch.cuda.synchronize()

    def write(self, **kw):
        """host arrays ([len, Bp] / [Bp], or [len, live] / [live] for the live columns only) into the device tensors"""
        for nm, v in kw.items():
            dst = getattr(self.be, nm)
            v = np.asarray(v)
            src = torch.from_numpy(np.ascontiguousarray(v.astype(np.int32 if dst.dtype == torch.int32 else self.P.T))).to(dev())
            if v.shape[-1] == self.Bp:
                dst.copy_(src)
            else:
                dst[..., torch.from_numpy(self.live).to(dev())] = src
        torch.cuda.synchronize()

    def tensors(self):
        be = self.be
        d = {nm: getattr(be, nm) for nm in XPOP + YPOP + SCAL + ("live", "action")}
        d.update({f"vec{i}": v for i, v in enumerate(be.vec) if v.dim() == 2})
        return d

    def snapshot(self):
        return {k: v.clone() for k, v in self.tensors().items()}

    def dead_unchanged(self, snap, what):
        idx = torch.from_numpy(self.dead).to(dev())
        for k, v in self.tensors().items():
            a, b = snap[k][..., idx].view(IVIEW[v.dtype]), v[..., idx].view(IVIEW[v.dtype])
            assert torch.equal(a, b), f"{what}: a frozen or padding column of {k} was written"

    def pull(self):
        self.be.synchronize()
        torch.cuda.synchronize()
        idx = torch.from_numpy(self.live).to(dev())
        st = {k: v[..., idx].double().cpu().numpy() for k, v in self.tensors().items() if not k.startswith("vec")}
        st["out"] = self.be.out[:, idx].cpu().numpy()
        for k in XPOP + YPOP + SCAL:
            assert np.isfinite(st[k]).all(), f"a live column of {k} is not finite"
        return st

    def call(self, what, fn, *args, **kw):
        """one entry point: the live state before, after, and the frozen / padding bytes checked"""
        before = self.pull()
        snap = self.snapshot()
        fn(*args, **kw)
        after = self.pull()
        self.dead_unchanged(snap, what)
        return before, after


def close(what, got, ref, err, c=C_BOUND):
    got, ref, err = (np.asarray(v, np.float64) for v in (got, ref, err))
    ok = np.abs(got - ref) <= c * err
    if not ok.all():
        i = np.flatnonzero(~ok.reshape(-1))[0]
        g, r, e = got.reshape(-1)[i], ref.reshape(-1)[i], err.reshape(-1)[i]
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} entries off, first [{i}]: got {g!r} want {r!r} "
                             f"(|diff| {abs(g - r):.3e} > {c} x {e:.3e})")


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 references with running-error bounds (u: the unit of the kernel's working precision)
# ---------------------------------------------------------------------------------------------------------------------------------
def gam(L, u):
    return (L + 1) * u


def ref_iterate(P, b, s, iters, adaptive, k0, u):
    """``iters`` iterations of column b from the state ``s`` (float64 vectors and scalars of that column, as the kernel holds them),
    the kernel's bookkeeping: fixed step x_sum += eta x+, eta_sum += eta; adaptive: x_sum += wpend x (the pending term of the
    iterate being left), eta_sum += eta_w, wpend = eta_w, eta = eta'.  Returns the new state and the bound ``e[name]`` of each."""
    o = P.oracle(b)
    c, q, l, hi = P.col(b)
    ineq = np.arange(P.m) < P.m_ineq
    s = dict(s)
    e = {k: np.zeros_like(np.asarray(s[k], np.float64)) for k in ("x", "y", "x_sum", "y_sum")}
    e.update(eta=0.0, eta_sum=0.0, wpend=0.0)
    om = s["omega"]
    s["accepted"] = []
    for it in range(iters):
        x, y, eta = s["x"], s["y"], s["eta"]
        ex, ey, ee = e["x"], e["y"], e["eta"]
        if adaptive:
            w = s["wpend"]
            s["x_sum"] = s["x_sum"] + w * x
            e["x_sum"] = e["x_sum"] + w * ex + e["wpend"] * np.abs(x) + 2 * u * (np.abs(w * x) + np.abs(s["x_sum"]))
        # primal half
        kty, akty = P.KT @ y, P.KTa @ np.abs(y)
        e_g = P.KTa @ ey + gam(P.Lc, u) * akty + u * (np.abs(c) + np.abs(kty))
        g = c - kty
        tau, e_tau = eta / om, ee / om + u * eta / om
        p = tau * g
        e_p = tau * e_g + e_tau * np.abs(g) + u * np.abs(p)
        v = x - p
        e_v = ex + e_p + u * (np.abs(x) + np.abs(p))
        clamped = (v + C_BOUND * e_v < l) | (v - C_BOUND * e_v > hi)      # projected with room to spare: exact
        if adaptive:
            xn, yn, eta_w, eta_h, info = o.step_adaptive(x, y, eta, om, 1.0, k0 + it + 1)
        else:
            xn, yn = o.step_fixed(x, y, eta, om, 1.0)
            eta_w = eta_h = eta
        e_xn = np.where(clamped, 0.0, e_v)
        xbar = xn + (xn - x)
        e_xbar = 2 * e_xn + ex + u * (np.abs(xn - x) + np.abs(xbar))
        # dual half
        kx = P.K @ xbar
        e_qk = P.Ka @ e_xbar + gam(P.Lr, u) * (P.Ka @ np.abs(xbar)) + u * (np.abs(q) + np.abs(kx))
        qk = q - kx
        sig, e_sig = eta * om, ee * om + u * eta * om
        sv = sig * qk
        e_s = sig * e_qk + e_sig * np.abs(qk) + u * np.abs(sv)
        wv = y + sv
        e_w = ey + e_s + u * (np.abs(y) + np.abs(sv))
        e_yn = np.where(ineq & (wv + C_BOUND * e_w < 0), 0.0, e_w)
        if adaptive:
            w = s["wpend"]
            s["y_sum"] = s["y_sum"] + w * y
            e["y_sum"] = e["y_sum"] + w * ey + e["wpend"] * np.abs(y) + 2 * u * (np.abs(w * y) + np.abs(s["y_sum"]))
            dx, dy = xn - x, yn - y
            e_dx = e_xn + ex + u * np.abs(dx)
            e_dy = e_yn + ey + u * np.abs(dy)
            kdy = P.KT @ dy
            e_kdy = P.KTa @ e_dy + gam(P.Lc, u) * (P.KTa @ np.abs(dy))
            dkd = float(kdy @ dx)
            e_dkd = float(np.abs(kdy) @ e_dx + e_kdy @ np.abs(dx) + e_kdy @ e_dx) + (P.n + 2) * U64 * float(np.abs(kdy * dx).sum())
            den = 2 * dkd
            e_den = 2 * (e_dkd + u * abs(dkd))
            den_o = float(info["denominator"])
            if den_o == 0.0:
                assert e_den == 0.0, "a zero denominator that is not exact: the test's inputs are ill-conditioned"
                e_ep = (ee / eta + 2 * u) * float(eta_h)
                accepted = True
            else:
                assert abs(den) > C_BOUND * e_den, "a denominator within its bound of 0: the test's inputs are ill-conditioned"
                dxx, dyy = float(dx @ dx), float(dy @ dy)
                e_dxx = float(2 * np.abs(dx) @ e_dx + e_dx @ e_dx) + (P.n + 2) * U64 * dxx + 3 * u * dxx
                e_dyy = float(2 * np.abs(dy) @ e_dy + e_dy @ e_dy) + (P.m + 2) * U64 * dyy + 3 * u * dyy
                num = om * dxx + dyy / om
                rel_bar = (om * e_dxx + e_dyy / om) / num + 3 * u + e_den / abs(den) + u
                eta_bar = float(info["eta_bar"])
                assert abs(eta - eta_bar) > C_BOUND * (ee + rel_bar * eta_bar), \
                    "eta within its bound of eta_bar: the test's inputs are ill-conditioned"
                t1 = (1.0 - (k0 + it + 2.0) ** -0.3) * eta_bar
                t2 = (1.0 + (k0 + it + 2.0) ** -0.6) * eta
                e1, e2 = (rel_bar + 2 * u) * t1, (ee / eta + 2 * u) * t2
                e_ep = e1 if t1 + e1 < t2 - e2 else e2 if t2 + e2 < t1 - e1 else max(e1, e2)     # min(t1, t2)
                accepted = bool(info["accepted"])
            s["accepted"].append(accepted)
            e_w_ = ee if accepted else e_ep
            s["eta_sum"] = s["eta_sum"] + float(eta_w)
            e["eta_sum"] = e["eta_sum"] + e_w_ + u * abs(s["eta_sum"])
            s["wpend"], e["wpend"] = float(eta_w), e_w_
            s["dy"], e["dy"] = dy, e_dy
            s["eta"], e["eta"] = float(eta_h), e_ep
        else:
            s["x_sum"] = s["x_sum"] + eta * xn
            e["x_sum"] = e["x_sum"] + eta * e_xn + 2 * u * (np.abs(eta * xn) + np.abs(s["x_sum"]))
            s["y_sum"] = s["y_sum"] + eta * yn
            e["y_sum"] = e["y_sum"] + eta * e_yn + 2 * u * (np.abs(eta * yn) + np.abs(s["y_sum"]))
        s["x_prev"], e["x_prev"] = x, ex
        s["y_prev"], e["y_prev"] = y, ey
        s["xbar"], e["xbar"] = xbar, e_xbar
        s["x"], e["x"] = xn, e_xn
        s["y"], e["y"] = yn, e_yn
    if not adaptive:
        for _ in range(iters):
            s["eta_sum"] = s["eta_sum"] + s["eta"]
            e["eta_sum"] = e["eta_sum"] + u * abs(s["eta_sum"])
    return s, e


def col_state(st, i):
    return {k: st[k][..., i] for k in XPOP + YPOP + SCAL}


def check_iterate(bt, before, after, iters, adaptive, k0, u, golden=None):
    """every live column after one pdlp_batch_iterate against ref_iterate; returns the accept flags of the adaptive rule"""
    flags = []
    names = ("x", "x_prev", "xbar", "x_sum", "y", "y_prev", "y_sum", "eta_sum") + (("dy", "eta", "wpend") if adaptive else ())
    for i, b in enumerate(bt.live):
        s, e = ref_iterate(bt.P, b, col_state(before, i), iters, adaptive, k0, u)
        for nm in names:
            close(f"iterate(iters={iters}, adaptive={adaptive}, k0={k0}) column {b} {nm}", after[nm][..., i], s[nm], e[nm])
        for nm in (("x_avg", "x_last", "y_avg", "y_last", "omega") + (() if adaptive else ("dy", "eta", "wpend"))):
            assert np.array_equal(after[nm][..., i], before[nm][..., i]), f"iterate wrote {nm} of column {b}"
        flags.append(s["accepted"])
    return flags


def ref_kkt(P, b, x, y, u, D=None):
    """the six sums of a KKT pass of column b at (x, y) (out[slot][b] in the order dr^2, l_dual'lam+, u_dual'lam-, c'x, pr^2, q'y)
    with their bounds; with D = (D_col, D_row) the sums of the un-scaled LP at (D_col x, D_row y), as the kernel forms them"""
    c, q, l, hi = P.col(b)
    kty = P.KT @ y
    e_g = gam(P.Lc, u) * (P.KTa @ np.abs(y)) + u * (np.abs(c) + np.abs(kty))
    g, cj, lo, up, xj = c - kty, c, l, hi, x
    e_c = e_lo = e_up = e_x = 0.0
    if D is not None:
        dc, dr = D
        g, e_g = g / dc, e_g / np.abs(dc) + u * np.abs(g / dc)
        cj, lo, up, xj = c / dc, l * dc, hi * dc, x * dc
        e_c, e_x = u * np.abs(cj), u * np.abs(xj)
        with np.errstate(invalid="ignore"):
            e_lo, e_up = np.where(np.isinf(lo), 0, u * np.abs(lo)), np.where(np.isinf(up), 0, u * np.abs(up))
    ninf, pinf = np.isneginf(lo), np.isposinf(up)
    lam = np.where(ninf & pinf, 0.0, np.where(ninf, np.minimum(g, 0), np.where(pinf, np.maximum(g, 0), g)))
    e_lam = np.where(ninf & pinf, 0.0, e_g)
    r = g - lam
    e_r = np.where(~ninf & ~pinf, 0.0, e_g)
    ld, ud = np.where(ninf, 0.0, lo), np.where(pinf, 0.0, up)
    e_ld, e_ud = np.where(ninf, 0.0, e_lo), np.where(pinf, 0.0, e_up)
    lp, ln = np.maximum(lam, 0), np.minimum(lam, 0)
    terms = [(r * r, 2 * np.abs(r) * e_r + e_r * e_r),
             (ld * lp, np.abs(ld) * e_lam + e_ld * np.abs(lp)),
             (ud * ln, np.abs(ud) * e_lam + e_ud * np.abs(ln)),
             (cj * xj, np.abs(xj) * e_c + np.abs(cj) * e_x)]
    kx = P.K @ x
    rr = kx - q
    e_rr = gam(P.Lr, u) * (P.Ka @ np.abs(x)) + u * (np.abs(kx) + np.abs(q))
    qi, yi, e_q, e_y = q, y, 0.0, 0.0
    if D is not None:
        rr, e_rr = rr / dr, e_rr / np.abs(dr) + u * np.abs(rr / dr)
        qi, yi = q / dr, y * dr
        e_q, e_y = u * np.abs(qi), u * np.abs(yi)
    rr = np.where((np.arange(P.m) < P.m_ineq) & (rr > 0), 0.0, rr)
    terms += [(rr * rr, 2 * np.abs(rr) * e_rr + e_rr * e_rr), (qi * yi, np.abs(yi) * e_q + np.abs(qi) * e_y)]
    S = np.array([t.sum() for t, _ in terms])
    E = np.array([ee.sum() + (t.size + 2) * U64 * np.abs(t).sum() for t, ee in terms])
    return S, E, np.array([np.abs(t).sum() for t, _ in terms])


def oracle_kkt_agrees(P, b, x, y, S, A, D=None):
    """the numpy sums above restate the oracle's KKT pass: its primal objective, residuals and adjusted dual from the same sums"""
    if D is None:
        o, xo, yo = P.oracle(b), x, y
    else:
        dc, dr = D
        c, q, l, u = P.col(b)
        Ku = sp.diags(1 / dr) @ P.K @ sp.diags(1 / dc)
        o = P.oracle(b, K=Ku.tocsr(), vec=(c / dc, q / dr, l * dc, u * dc))
        xo, yo = dc * x, dr * y
    k = o.kkt(xo, yo, 1.0)
    # float64 on both sides, other roundings of the un-scaled data: 1e-9 of the terms' sizes
    assert abs(float(k["p"]) - S[3]) <= 1e-9 * A[3], (b, float(k["p"]), S[3])
    assert abs(float(k["pr"]) ** 2 - S[4]) <= 1e-9 * A[4], (b, float(k["pr"]) ** 2, S[4])
    assert abs(float(k["dr"]) ** 2 - S[0]) <= 1e-9 * A[0], (b, float(k["dr"]) ** 2, S[0])
    assert abs(float(k["d_adj"]) - (S[5] + S[1] + S[2])) <= 1e-9 * (A[5] + A[1] + A[2]), b


def check_kkt(bt, st, which, slot, u, D=None, oracle_check=True):
    xn, yn = {N.CUR: ("x", "y"), N.AVG: ("x_avg", "y_avg"), N.PREV: ("x_prev", "y_prev")}[which]
    for i, b in enumerate(bt.live):
        x, y = st[xn][:, i], st[yn][:, i]
        S, E, A = ref_kkt(bt.P, b, x, y, u, D)
        close(f"kkt(which={which}, slot={slot}, unscaled={D is not None}) column {b}", st["out"][slot, i], S, E)
        if oracle_check:
            oracle_kkt_agrees(bt.P, b, x, y, S, A, D)


def check_average(bt, before, after, adaptive, u):
    for i, b in enumerate(bt.live):
        es = before["eta_sum"][i]
        for v in ("x", "y"):
            V, s = before[v][:, i], before[f"{v}_sum"][:, i]
            e_s = np.zeros_like(s)
            if adaptive:
                w = before["wpend"][i]
                s = s + w * V
                e_s = 2 * u * (np.abs(w * V) + np.abs(s))
            close(f"average(adaptive={adaptive}) column {b} {v}_sum", after[f"{v}_sum"][:, i], s, e_s)
            close(f"average(adaptive={adaptive}) column {b} {v}_avg", after[f"{v}_avg"][:, i], s / es, e_s / es + u * np.abs(s / es))
        want_w = 0.0 if adaptive else before["wpend"][i]
        assert after["wpend"][i] == want_w, f"average(adaptive={adaptive}): wpend of column {b}"
        for nm in ("x", "y", "x_prev", "y_prev", "xbar", "dy", "x_last", "y_last", "eta", "eta_sum", "omega"):
            assert np.array_equal(after[nm][..., i], before[nm][..., i]), f"average wrote {nm} of column {b}"


def check_restart(bt, before, after, actions, slot, u):
    """restarts with actions 0 / 1 / 2 mixed: the new point, zeroed sums, eta_sum and wpend, the marks, the squared distances"""
    for i, b in enumerate(bt.live):
        a = int(actions[b])
        if a == 0:
            for nm in XPOP + YPOP + SCAL:
                assert np.array_equal(after[nm][..., i], before[nm][..., i]), f"restart action 0 changed {nm} of column {b}"
            continue
        dist = []
        for v in ("x", "y"):
            new = before[f"{v}_avg" if a == 2 else v][:, i]
            assert np.array_equal(after[v][:, i], new), f"restart {a}: {v} of column {b}"
            assert np.array_equal(after[f"{v}_last"][:, i], new), f"restart {a}: {v}_last of column {b}"
            assert not after[f"{v}_sum"][:, i].any(), f"restart {a}: {v}_sum of column {b} not zeroed"
            d = new - before[f"{v}_last"][:, i]
            dist.append((float(d @ d), (d.size + 4) * u * float(d @ d)))
        assert after["eta_sum"][i] == 0.0 and after["wpend"][i] == 0.0, f"restart {a}: eta_sum / wpend of column {b}"
        close(f"restart {a} column {b} distances", after["out"][slot, i, :2], [dd for dd, _ in dist], [ee for _, ee in dist])
        for nm in ("x_prev", "xbar", "x_avg", "y_prev", "y_avg", "dy", "eta", "omega"):
            assert np.array_equal(after[nm][..., i], before[nm][..., i]), f"restart wrote {nm} of column {b}"


def units(T):
    return float(np.finfo(T).eps)


def run_cycle(bt, rng, iters=2, k0=3, kkt_oracle=True):
    """every entry point once in each mode, each call checked against the reference from the state the kernel left"""
    be, u = bt.be, units(bt.P.T)
    before, after = bt.call("iterate fixed", be.iterate, iters, False, 0)
    check_iterate(bt, before, after, iters, False, 0, u)
    before, after = bt.call("iterate adaptive", be.iterate, iters, True, k0)
    check_iterate(bt, before, after, iters, True, k0, u)
    before, after = bt.call("average adaptive", be.average, True)
    check_average(bt, before, after, True, u)
    before, after = bt.call("average fixed", be.average, False)
    check_average(bt, before, after, False, u)
    for which, slot in ((N.CUR, 0), (N.AVG, 1), (N.PREV, 2)):
        _, after = bt.call("kkt", be.kkt, which, slot)
        check_kkt(bt, after, which, slot, u, oracle_check=kkt_oracle)
    actions = np.zeros(bt.Bp, np.int32)
    actions[bt.live] = np.arange(len(bt.live)) % 3
    bt.write(action=actions)
    before, after = bt.call("restart", be.restart, 1)
    check_restart(bt, before, after, actions, 1, u)
    return after


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. steps
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("iters", [1, 7])
@pytest.mark.parametrize("adaptive", [False, True], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("k0", [0, 10**6])
def test_steps(T, iters, adaptive, k0):
    """column 0 the golden LP and start; the others perturbed c, q, bounds, starts, eta and omega: accepted and rejected adaptive
    steps in one launch"""
    rng = np.random.default_rng(100 + iters + 2 * adaptive + (k0 > 0))
    file = "step_adaptive.npz" if adaptive else "step_fixed.npz"
    P, g = golden_lp(T, 9, rng, file=file)
    # one step: eta up to 200 times the stable step, so that the rule rejects some; seven: steps the rule accepts all along (a
    # rejected step blows the iterate up, and the bound of the next step's denominator with it)
    spread = ((0.5, 200.0) if iters == 1 else (0.1, 0.6)) if adaptive else (0.2, 1.0)
    bt = Batch(P, 9, rng=rng, eta_spread=spread)
    a = lambda k: g[f"mixed_400x300/{k}"]
    st = bt.pull()
    st["x"][:, 0], st["y"][:, 0] = a("x0"), a("y0")
    st["omega"][0] = a("omega")
    if iters == 1:                        # seven adaptive steps from the golden eta are too ill-conditioned in float32 to bound
        st["eta"][0] = a("eta") if not adaptive else a("accept/eta_in")
    bt.write(x=st["x"], y=st["y"], omega=st["omega"], eta=st["eta"])
    before, after = bt.call("iterate", bt.be.iterate, iters, adaptive, k0)
    flags = check_iterate(bt, before, after, iters, adaptive, k0, units(T))
    if adaptive and iters == 1:
        first = [f[0] for f in flags]
        assert any(first) and not all(first), f"the launch must hold accepted and rejected steps: {first}"
    if not adaptive and iters == 1 and T == np.float32:          # the reference's own recorded step
        u = units(T)
        s, e = ref_iterate(P, 0, col_state(before, 0), 1, False, 0, u)
        close("golden x1", after["x"][:, 0], a("x1"), 2 * e["x"])
        close("golden y1", after["y"][:, 0], a("y1"), 2 * e["y"])


@pytest.mark.parametrize("group", ["accept", "reject", "late", "denzero"])
def test_golden_adaptive_step_columns(group):
    """the recorded adaptive steps (step_adaptive.npz) as column 0 of a float32 batch at their own k, perturbed columns beside"""
    T, B, u = np.float32, 8, units(np.float32)
    rng = np.random.default_rng(7)
    g = np.load(os.path.join(GOLDEN, "step_adaptive.npz"))
    if group == "denzero":
        r = lambda k: g[f"denzero/{k}"]
        Kd = r("K").astype(T)
        Ks = sp.csr_matrix(Kd)
        Ks.sort_indices()
        C = np.stack([r("c")] + [r("c") * rng.uniform(-1, 1, 6) for _ in range(1, B)], 1)
        P = LP(4, 6, int(r("m_ineq")), Ks.indptr, Ks.indices, Ks.data, C, r("q"), r("l"), r("u"), T=T)
        x0, y0, omega, k = np.zeros(6), np.zeros(4), r("omega"), int(r("k"))
        rec = dict(eta_in=r("eta_in"), x1=r("x1"), y1=r("y1"), eta_used=r("eta_used"), eta_hat=r("eta_hat"))
    else:
        P, _ = golden_lp(T, B, rng, per="CQlu", file="step_adaptive.npz")
        a = lambda k: g[f"mixed_400x300/{k}"]
        x0, y0, omega, k = a("x0"), a("y0"), a("omega"), int(a(f"{group}/k"))
        rec = {nm: a(f"{group}/{nm}") for nm in ("eta_in", "x1", "y1", "eta_used", "eta_hat")}
    bt = Batch(P, B, rng=rng, eta_spread=(0.2, 4.0))
    st = bt.pull()
    st["x"][:, 0], st["y"][:, 0], st["omega"][0], st["eta"][0] = x0, y0, omega, rec["eta_in"]
    bt.write(x=st["x"], y=st["y"], omega=st["omega"], eta=st["eta"])
    before, after = bt.call("iterate", bt.be.iterate, 1, True, k - 1)
    flags = check_iterate(bt, before, after, 1, True, k - 1, u)
    s, e = ref_iterate(P, 0, col_state(before, 0), 1, True, k - 1, u)
    close("golden x1", after["x"][:, 0], rec["x1"], 2 * e["x"])
    close("golden y1", after["y"][:, 0], rec["y1"], 2 * e["y"])
    close("golden eta_used", after["wpend"][0], rec["eta_used"], 2 * e["wpend"] + u * abs(rec["eta_used"]))
    close("golden eta_hat", after["eta"][0], rec["eta_hat"], 2 * e["eta"] + u * abs(rec["eta_hat"]))
    if group == "denzero":
        assert flags[0] == [True]


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. KKT, scaled and un-scaled with real Ruiz factors
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ruiz_lp(T, B):
    """the golden ruiz.npz LP equilibrated by the library's equilibrate_matrix in T: K_s, D_col, D_row and per-LP scaled vectors"""
    z = np.load(os.path.join(GOLDEN, "ruiz.npz"))
    Kd = z["mixed_400x300/plain/it20/K"].astype(np.float64)
    m, n = Kd.shape
    Kc = sp.csr_matrix(Kd)
    Kc.sort_indices()
    t = lambda a, dt=TORCH[T]: torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dt)
    Kp = tp.CsrPair(m, n, t(Kc.indptr, torch.int64), t(Kc.indices, torch.int32), t(Kc.data)).to(dev())
    Ks, scaling = tp.equilibrate_matrix(Kp, device=dev())
    torch.cuda.synchronize()
    rp, ci, va = (v.cpu().numpy() for v in (Ks.rowptr, Ks.colidx, Ks.val))
    dc, dr = scaling.d_col.double().cpu().numpy(), scaling.d_row.double().cpu().numpy()
    assert not np.allclose(dc, 1) and not np.allclose(dr, 1)
    rng = np.random.default_rng(5)
    L, U = bounds_mix(n, rng, np.float64, B)
    P = LP(m, n, int(0.6 * m), rp, ci, va, rng.standard_normal((n, B)), rng.standard_normal((m, B)), L, U, T=T)
    return P, (dc.astype(T).astype(np.float64), dr.astype(T).astype(np.float64))


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("which,slot", [(N.CUR, 0), (N.AVG, 2), (N.PREV, 1)], ids=["cur", "avg", "prev"])
@pytest.mark.parametrize("unscaled", [False, True], ids=["scaled", "unscaled"])
def test_kkt(T, which, slot, unscaled):
    B = 11
    P, D = ruiz_lp(T, B)
    bt = Batch(P, B, frozen=(4,), rng=np.random.default_rng(slot), D=D)
    _, after = bt.call("kkt", bt.be.kkt, which, slot, unscaled)
    check_kkt(bt, after, which, slot, units(T), D if unscaled else None)
    other = [s for s in range(3) if s != slot]
    assert not after["out"][other].any(), "a KKT pass wrote another slot"


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. average and restart
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("adaptive", [False, True], ids=["fixed", "adaptive"])
def test_average_then_restart_mixed(T, adaptive):
    rng = np.random.default_rng(31 + adaptive)
    P, _ = golden_lp(T, 10, rng)
    bt = Batch(P, 10, frozen=(3, 8), rng=rng)
    u = units(T)
    before, after = bt.call("average", bt.be.average, adaptive)
    check_average(bt, before, after, adaptive, u)
    actions = np.zeros(bt.Bp, np.int32)
    actions[bt.live] = [0, 1, 2, 2, 1, 0, 1, 2][:len(bt.live)]
    bt.write(action=actions)
    before, after = bt.call("restart", bt.be.restart, 2)
    check_restart(bt, before, after, actions, 2, u)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. edge shapes, shared and per-LP vectors; 7. frozen columns
# ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = ["1x1", "ineq0", "ineq_all", "empty_rows_cols", "long_row", "odd_rows"]
VECS = ["CQLU", "cqlu", "CqLU", "cQlu", "CQlU", "CQLu"]          # upper case: one column per LP, lower case: shared


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("per", VECS)
def test_shapes_and_vectors(shape, per):
    rng = np.random.default_rng(10 * SHAPES.index(shape) + VECS.index(per))
    B = 10
    P = shape_lp(shape, np.float32, B, per, rng)
    bt = Batch(P, B, frozen=(1, 6), rng=rng)
    run_cycle(bt, rng)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. widths and padding
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,W", [(np.float32, 1, None), (np.float32, 8, None), (np.float32, 9, None), (np.float32, 32, None),
                                   (np.float32, 33, None), (np.float32, 100, None), (np.float64, 1, None), (np.float64, 16, None),
                                   (np.float64, 17, None), (np.float64, 5, 32)])
def test_widths_and_padding(T, B, W):
    rng = np.random.default_rng(B)
    P, _ = golden_lp(T, B, rng)
    bt = Batch(P, B, W=W, rng=rng)
    assert bt.be.W == (W or group_width(B, TORCH[T]))
    run_cycle(bt, rng, kkt_oracle=B <= 17)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. grid-stride sizes
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big(T, B):
    return big_lp(T, B, np.random.default_rng(99))


@pytest.mark.parametrize("T,B,W", [(np.float32, 6, 8), (np.float32, 3, 32), (np.float64, 2, 16)], ids=["f32-W8", "f32-W32", "f64-W16"])
def test_grid_stride(T, B, W):
    P = big(T, B)
    rows_cap = 8192 * 4 * (64 // W)
    assert P.m > rows_cap and (W != 32 or P.n > rows_cap)
    rng = np.random.default_rng(W)
    bt = Batch(P, B, W=W, frozen=(1,), rng=rng)
    run_cycle(bt, rng, iters=1, kkt_oracle=False)


def test_grid_stride_bit_identity():
    """an LP's bits do not depend on its batch at this size either: the same LP at another position beside other LPs"""
    T, W = np.float32, 8
    P = big(T, 6)
    outs = []
    for cols in ([0, 2, 3], [4, 5, 0, 3]):
        Q = LP(P.m, P.n, P.m_ineq, P.rp, P.ci, P.va, P.vec[0][:, cols], P.vec[1], P.vec[2][:, cols], P.vec[3][:, cols], T=T)
        bt = Batch(Q, len(cols), W=W, rng=np.random.default_rng(1))
        st = bt.pull()
        pos = cols.index(0)
        base = Batch(P, 6, W=W, rng=np.random.default_rng(1)).pull()
        for nm in XPOP + YPOP:
            st[nm][:, pos] = base[nm][:, 0]
        for nm in SCAL:
            st[nm][pos] = base[nm][0]
        bt.write(**{nm: st[nm] for nm in XPOP + YPOP + SCAL})
        bt.be.iterate(3, True, 0)
        bt.be.kkt(N.CUR, 0)
        r = bt.pull()
        outs.append(({nm: r[nm][..., pos].copy() for nm in XPOP + YPOP + SCAL}, r["out"][0, pos].copy()))
        del bt
    (a, oa), (b, ob) = outs
    for nm in a:
        assert np.array_equal(np.asarray(a[nm]).view(np.uint64), np.asarray(b[nm]).view(np.uint64)), nm
    assert np.array_equal(oa.view(np.uint64), ob.view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. whole solves in float64 against oracle.pdlp_algorithm
# ---------------------------------------------------------------------------------------------------------------------------------
MODES = {"fixed": {}, "adaptive": dict(adaptive=True), "adaptive_pw": dict(adaptive=True, primal_update=True),
         "ruiz": dict(precondition=True)}


@functools.lru_cache(maxsize=None)
def whole_problem(mode):
    from tests.test_gpu_batch import golden_family, golden_oracle
    G = golden_family(dtype=np.float64)
    B = G["C"].shape[1]
    lps = [golden_oracle(G, b, np.float64) for b in range(B)]
    if mode == "ruiz":
        sc = [lp.ruiz() for lp in lps]
        data = [(s[1], s[2], lp) for s, lp in zip(sc, lps)]
        lps = [s[0] for s in sc]
    else:
        data = [None] * B
    sigma = float(lps[0].power_iter(G["b0"]))
    return G, lps, data, sigma


@functools.lru_cache(maxsize=None)
def oracle_solves(mode, max_kkt=100_000):
    from oracle import oracle as orc
    G, lps, data, sigma = whole_problem(mode)
    kw = dict(MODES[mode])
    return [orc.pdlp_algorithm(lp, sigma=sigma, max_kkt=max_kkt, data_precond=d, **kw) for lp, d in zip(lps, data)]


def batch_solve(mode, W=None, max_kkt=100_000):
    G, lps, data, sigma = whole_problem(mode)
    B = len(lps)
    t = lambda v, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(v)).to(device=dev(), dtype=dt)
    o = lps[0]
    K = tp.CsrPair(o.m, o.n, t(o.rp, torch.int64), t(o.ci, torch.int32), t(o.va))
    col = lambda a: t(np.stack([getattr(lp, a) for lp in lps], 1))
    traces = [dict(kkt=[], omega=[], restarts=[]) for _ in range(B)]
    kw = dict(MODES[mode])
    if mode == "ruiz":
        kw["data_precond"] = (t(data[0][0]), t(data[0][1]))
    out = pdlp_algorithm_batch(K, o.m_ineq, col("c"), col("q"), col("l"), col("u"), dev(), sigma=sigma, traces=traces,
                               group_width=W, max_kkt=max_kkt, **kw)
    return out, traces


def compare_solves(out, traces, ref, whole=True):
    """per LP: (k, n, j, status), the restart sequence, every trace KKT value and omega, the objective.  ``whole=False`` (the
    adaptive rule): the first two restart checks only, and the status.  The rule feeds the step size back through ratios of
    iterate differences, which amplifies rounding by about 100 per restart period on this family: two float64 runs of the oracle
    itself with different thread counts part at 1e-10 by the third check and take different restarts later."""
    _, _, obj, k, n, j, st, _ = out
    for b, (xo, po, ko, no, jo, so, _, tr) in enumerate(ref):
        mine = traces[b]
        if not whole:
            assert st[b] == so, b
            assert [tuple(r) for r in mine["restarts"][:2]] == [tuple(r) for r in tr["restarts"][:2]], b
            np.testing.assert_allclose(mine["kkt"][:8], tr["kkt"][:8], rtol=1e-9, err_msg=str(b))
            np.testing.assert_allclose(mine["omega"][:2], tr["omega"][:2], rtol=1e-9, err_msg=str(b))
            continue
        assert (int(k[b]), int(n[b]), int(j[b]), st[b]) == (ko, no, jo, so), b
        assert [tuple(r) for r in mine["restarts"]] == [tuple(r) for r in tr["restarts"]], b
        assert len(mine["kkt"]) == len(tr["kkt"]), b
        np.testing.assert_allclose(mine["kkt"], tr["kkt"], rtol=1e-9, err_msg=str(b))
        np.testing.assert_allclose(mine["omega"], tr["omega"], rtol=1e-9, err_msg=str(b))
        np.testing.assert_allclose(obj[b], po, rtol=1e-9, err_msg=str(b))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("W", [None, 16])
def test_whole_solve_float64(mode, W):
    out, traces = batch_solve(mode, W)
    compare_solves(out, traces, oracle_solves(mode), whole=not MODES[mode].get("adaptive", False))


def test_whole_solve_float64_kkt_cap_between_checks():
    """a max_kkt that some LPs reach between two restart checks while the others run on (fixed step: whole solves compare)"""
    full = oracle_solves("fixed")
    js = sorted(r[4] for r in full)
    cap = js[len(js) // 2] - 17
    ref = oracle_solves("fixed", cap)
    assert any(r[5] != "Solved" for r in ref) and any(r[5] == "Solved" for r in ref)
    out, traces = batch_solve("fixed", None, cap)
    compare_solves(out, traces, ref)


def test_frozen_lp_is_untouched_adaptive():
    """the adaptive counterpart of test_gpu_batch's test: LP 2 starts at its optimum and is solved at its first restart"""
    from tests.test_gpu_batch import family, run
    f = family(8, seed=21)
    x0, y0 = torch.zeros(f.n, 8), torch.zeros(f.m, 8)
    x0[:, 2], y0[:, 2] = f.X_opt[:, 2], f.Y_opt[:, 2]
    a = run(f, x_init=x0.to(dev()), y_init=y0.to(dev()), adaptive=True, primal_update=True)
    assert a[6][2] == "Solved" and a[4][2] == 1
    assert max(a[4][b] for b in range(8) if b != 2) >= 2
    alone = run(f, cols=[2], group_width=8, x_init=x0[:, 2:3].to(dev()), y_init=y0[:, 2:3].to(dev()), adaptive=True,
                primal_update=True)
    assert torch.equal(a[0][:, 2], alone[0][:, 0]) and torch.equal(a[1][:, 2], alone[1][:, 0])
    assert (a[3][2], a[4][2], a[5][2], a[6][2]) == (alone[3][0], alone[4][0], alone[5][0], alone[6][0])
