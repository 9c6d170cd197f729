"""The solution report (pdlp_report_local, pdlp_batch_report and everything above them) on the GPU.

Call by call, in the convention of tests/test_gpu_batch_kernels.py: every stored entry and every sum is compared with float64
numpy on the same inputs within ``C_BOUND`` times a running-error bound of the kernel's own arithmetic, carried through the
operation entry by entry.  With u the unit of the working precision: a product ``sum_j K_ij v_j`` over a row of L items may be off
by ``(L + 1) u sum_j |K_ij| |v_j|`` (L multiplications, L - 1 additions in any order, one more for the tiled kernels' remainder);
every other rounding adds u times the size of its result; errors pass through the projections with factor 1 (they are
1-Lipschitz); a double sum of len terms adds ``(len + 2) u64`` times the sum of the terms' sizes.  ``C_BOUND = 4``: 2 for the
reference's own roundings, 2 for second-order terms.  Nothing is skipped: every entry of every vector is compared.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import torchpdlp_amd as tp
from torchpdlp_amd import _native as N
from torchpdlp_amd.batch import BatchEngine
from torchpdlp_amd.solver import run_pdlp
from torchpdlp_amd.tiled import build_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AFIRO = os.path.join(ROOT, "tests", "golden", "mps", "afiro.mps")
C_BOUND = 4.0
U64 = np.finfo(np.float64).eps
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
POISON = {np.float32: (np.uint32, 0x7FA5A5A5), np.float64: (np.uint64, 0x7FF4A5A5A5A5A5A5)}
IVIEW = {torch.float32: torch.int32, torch.float64: torch.int64}
RUIZ_ROUNDINGS = 2 * 20 + 4     # an entry of the scaled matrix: at most two divisions per sweep (20 sweeps), a factor D one per sweep


def dev():
    return torch.device("cuda", 0)


def h64(t):
    return t.detach().cpu().double().numpy().reshape(-1)


class LP:
    """an LP in float64 numpy whose numbers are values of the working precision T (matrix: of Tm)"""

    def __init__(self, m, n, m_ineq, rp, ci, va, c, q, l, u, T, Tm=None, dcol=None, drow=None):
        Tm = T if Tm is None else Tm
        self.m, self.n, self.m_ineq, self.T, self.Tm = int(m), int(n), int(m_ineq), T, Tm
        self.rp, self.ci, self.va = np.asarray(rp, np.int64), np.asarray(ci, np.int32), np.asarray(va, Tm).astype(np.float64)
        mk = lambda v: sp.csr_matrix((v, self.ci.copy(), self.rp.copy()), shape=(self.m, self.n))
        self.K, self.Ka = mk(self.va), mk(np.abs(self.va))
        self.Lr = np.diff(self.rp).astype(np.float64)
        self.Lc = np.bincount(self.ci, minlength=self.n).astype(np.float64)
        r = lambda v: None if v is None else np.asarray(v, T).astype(np.float64)
        self.c, self.q, self.l, self.u, self.dcol, self.drow = r(c), r(q), r(l), r(u), r(dcol), r(drow)

    def csr(self):
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dt)
        return tp.CsrPair(self.m, self.n, t(self.rp, torch.int64), t(self.ci, torch.int32), t(self.va, TORCH[self.Tm])).to(dev())

    def vec(self, name):
        v = getattr(self, name)
        return None if v is None else torch.from_numpy(v).to(TORCH[self.T]).to(dev())


def make_lp(T, rng, m=900, n=700, m_ineq=400, Tm=None, scaled=True):
    """~4 items per row; row 0 and column 5 hold nothing, row 3 holds column 9 twice; every bound class of project_lambda_box"""
    live = np.setdiff1d(np.arange(n), [5])
    rows = [[] if i == 0 else np.sort(rng.choice(live, 3 + i % 3, replace=False)) for i in range(m)]
    rows[3] = np.sort(np.concatenate([rows[3], [9, 9]]))
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.concatenate([np.asarray(r, np.int64) for r in rows]).astype(np.int32)
    va = (rng.uniform(0.2, 2.0, ci.size) * rng.choice([-1, 1], ci.size)).astype(np.float32)       # float32 numbers in every precision
    kind = rng.integers(0, 4, n)                     # boxed, lower only, upper only, free
    lo = rng.uniform(-2, 0, n)
    l = np.where(kind >= 2, -np.inf, lo)
    u = np.where((kind == 1) | (kind == 3), np.inf, lo + rng.uniform(0.5, 3, n))
    dcol = rng.uniform(0.5, 2.0, n) if scaled else None
    drow = rng.uniform(0.5, 2.0, m) if scaled else None
    return LP(m, n, m_ineq, rp, ci, va, rng.standard_normal(n), rng.standard_normal(m), l, u, T, Tm, dcol, drow)


def ref_report(P, x, y, unscaled, u, c=None, q=None, l=None, uu=None, extra=0.0):
    """(lam, act, sums[6]) in float64 and their running-error bounds for arithmetic with unit u; ``extra``: roundings every
    matrix entry and scaling factor already carries (a Ruiz-scaled problem evaluated against the original one)"""
    c, q, l, uu = (P.c if c is None else c), (P.q if q is None else q), (P.l if l is None else l), (P.u if uu is None else uu)
    n, m = P.n, P.m
    kty, e_kty = P.K.T @ y, (P.Lc + 1 + extra) * u * (P.Ka.T @ np.abs(y))
    kx, e_kx = P.K @ x, (P.Lr + 1 + extra) * u * (P.Ka @ np.abs(x))
    g = c - kty
    e_g = e_kty + u * np.abs(g)
    cj, lo, hi, xj = c, l, uu, x
    z = np.zeros(n)
    e_c, e_lo, e_hi, e_x = z, z, z, z
    fin = lambda v: np.where(np.isfinite(v), np.abs(v), 0.0)
    if unscaled:
        d = P.dcol
        g = g / d
        e_g = e_g / d + u * np.abs(g)
        cj, lo, hi, xj = c / d, l * d, uu * d, x * d
        e_c, e_lo, e_hi, e_x = u * np.abs(cj), u * fin(lo), u * fin(hi), u * np.abs(xj)
    ninf, pinf = np.isneginf(lo), np.isposinf(hi)
    lam = np.where(ninf & pinf, 0.0, np.where(ninf, np.minimum(g, 0), np.where(pinf, np.maximum(g, 0), g)))
    e_lam = np.where(ninf & pinf, 0.0, e_g)
    ld, ud = np.where(ninf, 0.0, lo), np.where(pinf, 0.0, hi)
    r = g - lam
    e_r = e_g + e_lam + u * np.abs(r)
    dsum = lambda terms: (len(terms) + 2) * U64 * np.abs(terms).sum()
    lp_, lm_ = np.maximum(lam, 0), np.minimum(lam, 0)
    s = np.zeros(6)
    b = np.zeros(6)
    s[0], b[0] = (r * r).sum(), (2 * np.abs(r) * e_r + e_r ** 2).sum() + dsum(r * r)
    s[1], b[1] = (ld * lp_).sum(), (np.abs(ld) * e_lam + e_lo * (np.abs(lp_) + e_lam)).sum() + dsum(ld * lp_)
    s[2], b[2] = (ud * lm_).sum(), (np.abs(ud) * e_lam + e_hi * (np.abs(lm_) + e_lam)).sum() + dsum(ud * lm_)
    s[3], b[3] = (cj * xj).sum(), (e_c * np.abs(xj) + e_x * np.abs(cj) + e_c * e_x).sum() + dsum(cj * xj)
    rr = kx - q
    e_rr = e_kx + u * np.abs(rr)
    qi, yi, act, e_act = q, y, kx, e_kx
    zm = np.zeros(m)
    e_q, e_y = zm, zm
    if unscaled:
        d = P.drow
        rr = rr / d
        e_rr = e_rr / d + u * np.abs(rr)
        qi, yi, act = q / d, y * d, kx / d
        e_q, e_y, e_act = u * np.abs(qi), u * np.abs(yi), e_kx / d + u * np.abs(act)
    rr = np.where((np.arange(m) < P.m_ineq) & (rr > 0), 0.0, rr)
    s[4], b[4] = (rr * rr).sum(), (2 * np.abs(rr) * e_rr + e_rr ** 2).sum() + dsum(rr * rr)
    s[5], b[5] = (qi * yi).sum(), (e_q * np.abs(yi) + e_y * np.abs(qi) + e_q * e_y).sum() + dsum(qi * yi)
    return lam, act, s, e_lam, e_act, b


def assert_within(got, want, bound, what, worst=None):
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = np.abs(got - want)
    ratio = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)), initial=0.0))
    print(f"{what}: max error / bound = {ratio:.3g}")
    if worst is not None:
        worst.append(ratio)
    assert (err <= C_BOUND * bound).all(), f"{what}: error / bound up to {ratio:.3g} (allowed {C_BOUND})"


# ---------------------------------------------------------------------------------------------------------------------------------
# pdlp_report_local, call by call
# ---------------------------------------------------------------------------------------------------------------------------------
def build_engine(P, family, mixed=False, delta=None):
    K = P.csr()
    vd = torch.float64 if mixed else None
    eng = tp.PdlpEngine(K.m, K.n, P.m_ineq, (K.rowptr, K.colidx, K.val), (K.t_rowptr, K.t_colidx, K.t_val), P.vec("c"), P.vec("q"),
                        P.vec("l"), P.vec("u"), d_col=P.vec("dcol"), d_row=P.vec("drow"), vec_dtype=vd, delta=delta, tiles=False)
    if family == "sorted":
        for tr in (0, 1):
            eng.attach_sorted(tr, True, force=True)
            assert eng.kernels[tr].startswith("csr, sorted")
    elif family == "tiled":
        for tr, (rp, ci, va), rows, cols in ((0, eng.K, P.m, P.n), (1, eng.KT, P.n, P.m)):
            t = build_tiles(rp, ci, va, rows, cols, lw=7)
            assert t is not None and t.npanel > 1
            eng.attach_tiles(tr, t)
            assert eng.kernels[tr].startswith("tiled")
    return eng


def prepare_iterates(eng, P, rng):
    """a few steps from a random point, then the average: CUR, AVG and PREV all hold something"""
    T = TORCH[P.T]
    x0 = torch.from_numpy(np.clip(rng.uniform(-1.5, 1.5, P.n), P.l, P.u)).to(T).to(dev())
    y0 = rng.uniform(-1, 1, P.m)
    y0[:P.m_ineq] = np.abs(y0[:P.m_ineq])
    eng.set_iterate(x0, torch.from_numpy(y0).to(T).to(dev()))
    eng.set_step(0.05, 1.3, 1.0, 0)
    eng.iterate(3, False)
    eng.flush_average(False)
    eng.compute_average()


def raw_report(eng, which, unscaled, want_rc=True, want_act=True):
    rc = torch.empty(eng.nl, dtype=eng.dtype, device=eng.device) if want_rc else None
    act = torch.empty(eng.ml, dtype=eng.dtype, device=eng.device) if want_act else None
    N.check(eng.lib.pdlp_report_local(eng.h, which, int(unscaled), None if rc is None else rc.data_ptr(),
                                      None if act is None else act.data_ptr()), "pdlp_report_local")
    red = (N.C.c_double * N.NRED)()
    N.check(eng.lib.pdlp_read_red(eng.h, red), "pdlp_read_red")
    return rc, act, np.array(red[:6])


def check_all_iterates(eng, P, u, kkt_too, worst=None):
    for which in (N.CUR, N.AVG, N.PREV):
        x, y = (h64(v) for v in eng.get_iterate(which))
        for unscaled in (0, 1):
            lam, act, s, e_lam, e_act, b = ref_report(P, x, y, unscaled, u)
            tag = f"which={which} unscaled={unscaled}"
            rc_d, act_d, red = raw_report(eng, which, unscaled)
            assert_within(h64(rc_d), lam, e_lam, f"reduced costs {tag}", worst)
            assert_within(h64(act_d), act, e_act, f"row activity {tag}", worst)
            assert_within(red, s, b, f"sums {tag}", worst)
            # a vector the caller does not ask for is not stored; the sums are the same sums
            _, act_only, red_a = raw_report(eng, which, unscaled, want_rc=False)
            rc_only, _, red_r = raw_report(eng, which, unscaled, want_act=False)
            assert torch.equal(act_only, act_d) and torch.equal(rc_only, rc_d)
            assert_within(red_a, s, b, f"sums without reduced costs {tag}")
            assert_within(red_r, s, b, f"sums without activities {tag}")
            if kkt_too:
                N.check(eng.lib.pdlp_kkt_local(eng.h, which, unscaled), "pdlp_kkt_local")
                red_k = (N.C.c_double * N.NRED)()
                N.check(eng.lib.pdlp_read_red(eng.h, red_k), "pdlp_read_red")
                assert_within(np.array(red_k[:6]), s, b, f"pdlp_kkt_local's sums {tag}")
                assert_within(red, np.array(red_k[:6]), 2 * b, f"report against pdlp_kkt_local {tag}")


@pytest.mark.parametrize("m_ineq", [0, 400, 900])
@pytest.mark.parametrize("family", ["csr", "sorted", "tiled"])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_report_local_against_float64(T, family, m_ineq):
    rng = np.random.default_rng(11 + m_ineq)
    P = make_lp(T, rng, m_ineq=m_ineq)
    eng = build_engine(P, family)
    prepare_iterates(eng, P, rng)
    check_all_iterates(eng, P, np.finfo(T).eps, kkt_too=True)


@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("family", ["csr", "tiled"])
def test_report_local_mixed_precision_is_exact_to_float64(family, delta):
    """float64 vectors over the float32-valued matrix: the float64-accumulated products, never the anchors of delta mode"""
    rng = np.random.default_rng(5)
    P = make_lp(np.float64, rng, Tm=np.float32)
    eng = build_engine(P, family, mixed=True, delta=delta)
    assert eng.mixed and eng.delta == delta
    prepare_iterates(eng, P, rng)
    check_all_iterates(eng, P, U64, kkt_too=not delta)


def test_report_local_rejects_what_it_cannot_do():
    rng = np.random.default_rng(1)
    P = make_lp(np.float32, rng, m=40, n=30, m_ineq=10, scaled=False)
    eng = build_engine(P, "csr")
    assert eng.lib.pdlp_report_local(eng.h, 5, 0, None, None) == -1
    assert eng.lib.pdlp_report_local(eng.h, -1, 0, None, None) == -1
    assert eng.lib.pdlp_report_local(eng.h, 0, 1, None, None) == -3           # un-scaled without d_col / d_row


# ---------------------------------------------------------------------------------------------------------------------------------
# the report changes nothing
# ---------------------------------------------------------------------------------------------------------------------------------
def solve_with_reports(lp, K, adaptive, mixed, with_reports):
    cast = (lambda t: t.double()) if mixed else (lambda t: t)
    eng = tp.PdlpEngine.from_full(K, cast(lp.c), cast(lp.q), cast(lp.l), cast(lp.u), lp.m_ineq, vec_dtype=torch.float64 if mixed else None)
    assert eng.delta == mixed
    calls = [0]
    if with_reports:
        kkt = eng.kkt

        def kkt_and_reports(which, omega, unscaled=False):
            for w in (N.CUR, N.AVG):
                eng.report(w)
            out = kkt(which, omega, unscaled)
            for w in (N.AVG, N.CUR):
                eng.report(w)
            calls[0] += 4
            return out
        eng.kkt = kkt_and_reports
    trace = dict(kkt=[], omega=[], restarts=[])
    x, obj, k, n, j, status, _ = run_pdlp(eng, tol=1e-6 if mixed else 1e-4, verbose=False, primal_update=True, adaptive=adaptive, sigma=3.0,
                                          trace=trace, max_kkt=6000)
    _, y = eng.get_iterate(N.CUR)
    return x.clone(), y.clone(), obj, k, n, j, status, trace, calls[0]


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("adaptive", [False, True])
def test_reports_during_a_solve_change_no_bit(adaptive, mixed):
    lp = tp.gen_lp(500, 400, 4, seed=3, device=dev(), recipe="mixed")
    K = tp.CsrPair(lp.m, lp.n, lp.rowptr, lp.colidx, lp.val)
    a = solve_with_reports(lp, K, adaptive, mixed, False)
    b = solve_with_reports(lp, K, adaptive, mixed, True)
    assert b[8] > 8 and a[8] == 0
    assert torch.equal(a[0].view(IVIEW[a[0].dtype]), b[0].view(IVIEW[b[0].dtype]))
    assert torch.equal(a[1].view(IVIEW[a[1].dtype]), b[1].view(IVIEW[b[1].dtype]))
    assert a[2:7] == b[2:7] and a[7] == b[7]


# ---------------------------------------------------------------------------------------------------------------------------------
# pdlp_batch_report
# ---------------------------------------------------------------------------------------------------------------------------------
def poison(shape, T):
    it, bits = POISON[T]
    return torch.from_numpy(np.full(shape, bits, dtype=it).view(T).copy())


@pytest.mark.parametrize("unscaled", [0, 1])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_batch_report_against_float64_and_touches_nothing_else(T, unscaled):
    rng = np.random.default_rng(23)
    B, Bp = 5, 8
    P = make_lp(T, rng, m=230, n=170, m_ineq=90)
    per = lambda v, ln: np.stack([v * (1 + 0.3 * rng.standard_normal(ln)) for _ in range(B)], 1).astype(T)
    Cb, Qb = per(P.c, P.n), per(P.q, P.m)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    be = BatchEngine(P.csr(), P.m_ineq, tt(Cb), tt(Qb), P.vec("l"), P.vec("u"), B, d_col=P.vec("dcol"), d_row=P.vec("drow"), W=8)
    assert be.Bp == Bp
    pops = {}
    for names, ln in ((("x", "x_prev", "xbar", "x_sum", "x_avg", "x_last"), P.n), (("y", "y_prev", "y_sum", "y_avg", "y_last", "dy"), P.m)):
        for nm in names:
            v = poison((ln, Bp), T)
            v[:, :B] = torch.from_numpy(rng.uniform(-1, 1, (ln, B)).astype(T))
            getattr(be, nm).copy_(v)
            pops[nm] = getattr(be, nm).clone()
    for nm in ("eta", "omega", "eta_sum", "wpend"):
        getattr(be, nm).copy_(poison((Bp,), T))
        pops[nm] = getattr(be, nm).clone()
    live = np.zeros(Bp, np.int32)
    live[[0, 2]] = 1                              # LPs 1, 3, 4 are frozen and reported all the same; 5..7 are padding
    be.live.copy_(torch.from_numpy(live))
    be.out.copy_(poison((3, Bp, 6), np.float64))
    out0 = be.out.clone()
    torch.cuda.synchronize()
    u = np.finfo(T).eps
    for slot, which in enumerate((N.CUR, N.AVG, N.PREV)):
        rc, act = poison((P.n, Bp), T).to(dev()), poison((P.m, Bp), T).to(dev())
        torch.cuda.synchronize()
        N.check(be.lib.pdlp_batch_report(be.eng.h, N.C.byref(be.desc), which, unscaled, slot, rc.data_ptr(), act.data_ptr()), "pdlp_batch_report")
        be.synchronize()
        out = be.out.cpu().numpy()
        X = h64(pops[("x", "x_avg", "x_prev")[which]]).reshape(P.n, Bp)
        Y = h64(pops[("y", "y_avg", "y_prev")[which]]).reshape(P.m, Bp)
        for b in range(B):
            lam, a, s, e_lam, e_act, bd = ref_report(P, X[:, b], Y[:, b], unscaled, u, c=Cb[:, b].astype(np.float64), q=Qb[:, b].astype(np.float64))
            assert_within(h64(rc[:, b]), lam, e_lam, f"batch reduced costs LP {b} which={which}")
            assert_within(h64(act[:, b]), a, e_act, f"batch row activity LP {b} which={which}")
            assert_within(out[slot, b], s, bd, f"batch sums LP {b} which={which}")
        iv = IVIEW[TORCH[T]]
        assert torch.equal(rc[:, B:].contiguous().view(iv), poison((P.n, Bp - B), T).to(dev()).view(iv))
        assert torch.equal(act[:, B:].contiguous().view(iv), poison((P.m, Bp - B), T).to(dev()).view(iv))
        assert torch.equal(be.out[slot, B:].contiguous().view(torch.int64), out0[slot, B:].contiguous().view(torch.int64))
        assert torch.equal(be.out[slot + 1:].contiguous().view(torch.int64), out0[slot + 1:].contiguous().view(torch.int64))
        for nm, before in pops.items():            # every population and scalar, every column: the same bytes
            assert torch.equal(getattr(be, nm).view(iv), before.view(iv)), nm
    b0 = N.PdlpBatch()
    assert be.lib.pdlp_batch_report(be.eng.h, N.C.byref(be.desc), 5, 0, 0, None, None) == -1
    assert be.lib.pdlp_batch_report(be.eng.h, N.C.byref(be.desc), 0, 0, 3, None, None) == -1
    assert be.lib.pdlp_batch_report(be.eng.h, N.C.byref(b0), 0, 0, 0, None, None) == -1


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def original_problem(problem, dtype):
    c, K, q, m_ineq, l, u = tp.api.load_problem(problem, dev(), dtype)
    T = np.float32 if dtype == torch.float32 else np.float64
    P = LP(K.m, K.n, m_ineq, h64(K.rowptr), h64(K.colidx), K.val.cpu().numpy(), h64(c), h64(q), h64(l), h64(u), T, Tm=T)
    P.orig = (c, K, q, m_ineq, l, u)
    return P, P.orig


def termination_norms(P, precondition):
    """||q||, ||c|| as the solver's check_termination is given them (pdhg.py:19-20,173), in float64 numpy: of the original q and c,
    or -- with preconditioning, as in the reference -- of q * D_row and c * D_col (enhancements.py:64-65) with the Ruiz factors of
    the original K.  The factors are a function of the original problem alone (K in fact); they come from equilibrate_matrix, the
    one place that defines them (its own tests: test_gpu_parity.py against tests/golden/ruiz.npz)."""
    if not precondition:
        return np.linalg.norm(P.q), np.linalg.norm(P.c)
    scaling = tp.equilibrate_matrix(P.orig[1], device=dev())[1]
    return np.linalg.norm(P.q * h64(scaling.d_row)), np.linalg.norm(P.c * h64(scaling.d_col))


def check_result_against_the_original_problem(res, P, precondition, tol, u, worst=None):
    """every report field from the returned x and y alone, float64 numpy on the original (c, K, q, l, u)"""
    assert res.y.shape == (P.m, 1) and res.reduced_costs.shape == (P.n, 1) and res.row_activity.shape == (P.m, 1)
    x, y = h64(res.x), h64(res.y)
    extra = RUIZ_ROUNDINGS if precondition else 0.0
    lam, act, s, e_lam, e_act, b = ref_report(P, x, y, 0, u, extra=extra)
    # x and y themselves are roundings of D_col x_s, D_row y_s: one more rounding in every term they enter (covered by extra + 1)
    assert_within(h64(res.reduced_costs), lam, e_lam, "reduced_costs", worst)
    assert_within(h64(res.row_activity), act, e_act, "row_activity", worst)
    if precondition:       # c_u = c_s / D_col ... are roundings of roundings: one u per factor of every term of the objective sums
        b = b + (2 + extra) * u * np.array([0, abs(s[1]), abs(s[2]), np.abs(P.c * x).sum(), 0, np.abs(P.q * y).sum()])
    p, d = s[3], s[5] + s[1] + s[2]
    e_p, e_d = b[3] + u * abs(p), b[5] + b[1] + b[2] + 3 * u * (abs(s[5]) + abs(s[1]) + abs(s[2]))
    root = lambda v, e: (np.sqrt(v), min(np.sqrt(C_BOUND * e), e / max(np.sqrt(v), 1e-300)) + u * np.sqrt(v))
    pr, e_pr = root(s[4], b[4])
    dr, e_dr = root(s[0], b[0])
    gap, e_gap = d - p, e_p + e_d + u * (abs(d) + abs(p))
    # the solver forms q_s, c_s in working precision (one rounding per entry) and rounds the norm to it: 3 u on the quotients
    qn, cn = termination_norms(P, precondition)
    e_pr0, e_dr0 = e_pr, e_dr
    e_pr, e_dr = e_pr + 3 * u * pr, e_dr + 3 * u * dr
    den = 1 + abs(p) + abs(d)
    for name, want, e in (("objective", p, e_p), ("dual_objective", d, e_d), ("primal_residual", pr, e_pr0), ("dual_residual", dr, e_dr0),
                          ("gap", gap, e_gap), ("rel_primal_residual", pr / (1 + qn), e_pr / (1 + qn)),
                          ("rel_dual_residual", dr / (1 + cn), e_dr / (1 + cn)),
                          ("rel_gap", gap / den, e_gap / den + abs(gap) * (e_p + e_d) / den ** 2)):
        assert_within(getattr(res, name), want, e + U64 * abs(want), name, worst)
    # "Solved" means the three relative figures pass tol; the exit test ran in working precision, possibly on carried products: the
    # same rounding on top.  Returned (not asserted here) so that a caller checks everything else of every LP first.
    missed = []
    if res.status == "Solved":
        for name, allow in (("rel_primal_residual", C_BOUND * e_pr / (1 + qn)), ("rel_dual_residual", C_BOUND * e_dr / (1 + cn)),
                            ("rel_gap", C_BOUND * (e_gap / den + abs(gap) * (e_p + e_d) / den ** 2))):
            print(f"Solved: {name} = {getattr(res, name):.6g} against tol = {tol:g} + {allow:.3g}")
            if not getattr(res, name) <= tol + allow:
                missed.append(f"{name} = {getattr(res, name):.6g} > {tol:g} + {allow:.3g}")
    return missed


def small_lp(dtype):
    lp = tp.gen_lp(300, 240, 4, seed=8, device=dev(), recipe="mixed", dtype=dtype)
    return (lp.c, tp.CsrPair(lp.m, lp.n, lp.rowptr, lp.colidx, lp.val), lp.q, lp.m_ineq, lp.l, lp.u), lp


@pytest.mark.parametrize("precondition", [False, True])
@pytest.mark.parametrize("mode", ["float32", "mixed"])
@pytest.mark.parametrize("which_lp", ["afiro", "gen_lp"])
def test_solve_lp_report_is_reproducible_from_x_and_y(which_lp, mode, precondition):
    mixed = mode == "mixed"
    dtype, tol = (torch.float64, 1e-8) if mixed else (torch.float32, 1e-4)
    problem = AFIRO if which_lp == "afiro" else small_lp(dtype)[0]
    kw = dict(tol=tol, precondition=precondition, primal_weight_update=True, adaptive_stepsize=True, seed=3, max_kkt=2_000_000,
              precision="mixed" if mixed else None)
    res = tp.solve_lp(problem, **kw)
    assert res.status == "Solved"
    P, orig = original_problem(problem, dtype)
    u = U64 if mixed else np.finfo(np.float32).eps
    missed = check_result_against_the_original_problem(res, P, precondition, tol, u)
    assert len(res.as_tuple()) == 7
    off = tp.solve_lp(problem, report=False, **kw)
    assert off.y is None and off.rel_gap is None and torch.equal(off.x, res.x) and off.kkt_passes == res.kkt_passes
    if which_lp == "afiro":
        opt = pytest.importorskip("scipy.optimize")
        A = P.K
        mi = P.m_ineq
        hi = opt.linprog(P.c, A_ub=-A[:mi], b_ub=-P.q[:mi], A_eq=A[mi:], b_eq=P.q[mi:], bounds=list(zip(P.l, P.u)), method="highs")
        assert hi.status == 0 and abs(res.dual_objective - hi.fun) <= 1e-3 * (1 + abs(hi.fun))
    assert not missed, missed


def test_a_run_stopped_by_the_pass_limit_still_reports():
    problem, lp = small_lp(torch.float32)
    res = tp.solve_lp(problem, tol=1e-9, max_kkt=200, seed=3, precondition=True)
    assert res.status == tp.STATUS_KKT_LIMIT and res.kkt_passes >= 200
    P, _ = original_problem(problem, torch.float32)
    check_result_against_the_original_problem(res, P, True, 1e-9, np.finfo(np.float32).eps)
    assert res.rel_primal_residual > 1e-9 or res.rel_dual_residual > 1e-9 or res.rel_gap > 1e-9


def test_batch_report_columns_match_single_solves():
    """Every column of a preconditioned batch and the single solve of the same LP: all report fields reproduce from x and y on the
    original problem, and "Solved" means rel_* <= tol (against the norms of the scaled q and c: the exit test's own, see
    termination_norms -- for LP 3 of this family ||c_s|| = 376.0 against ||c|| = 16.74)."""
    f = tp.gen_lp_family(120, 90, 4, 4, seed=2, device=dev())
    B = f.C.shape[1]
    prob = (f.C[:, 0], tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val), f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0])
    kw = dict(tol=1e-4, primal_weight_update=True, adaptive_stepsize=True, seed=1, precondition=True)
    res = tp.solve_lp_batch(prob, c=f.C, q=f.Q, l=f.L, u=f.U, **kw)
    assert len(set(int(k) for k in res.iterations)) > 1                      # the LPs finish at different checks
    assert res.reduced_costs.shape == (f.n, B) and res.row_activity.shape == (f.m, B)
    assert tp.solve_lp_batch(prob, c=f.C, q=f.Q, l=f.L, u=f.U, report=False, **kw).reduced_costs is None
    u = np.finfo(np.float32).eps
    missed = []
    for i in range(len(res)):
        one_prob = (f.C[:, i], prob[1], f.Q[:, i], f.m_ineq, f.L[:, i], f.U[:, i])
        P, _ = original_problem(one_prob, torch.float32)
        r = res[i]
        assert r.status == "Solved"
        missed += [f"batch LP {i}: {v}" for v in check_result_against_the_original_problem(r, P, True, 1e-4, u)]
        single = tp.solve_lp(one_prob, **kw)
        missed += [f"single LP {i}: {v}" for v in check_result_against_the_original_problem(single, P, True, 1e-4, u)]
        # two solves of one LP stop at points of their own: both reports describe an optimum to the tolerance
        assert abs(r.dual_objective - single.dual_objective) <= 2e-4 * (1 + abs(r.objective) + abs(r.dual_objective)) + 2e-4 * (
            1 + abs(single.objective) + abs(single.dual_objective)) + abs(r.objective - single.objective)
    assert not missed, missed


def test_cli_solution_dir(tmp_path):
    import shutil
    from torchpdlp_amd.__main__ import main
    one = tmp_path / "in"
    one.mkdir()
    shutil.copy(AFIRO, one / "afiro.mps")
    args = ["--instance_path", str(one), "--output_path", str(tmp_path / "out"), "--adaptive_stepsize", "--primal_weight_update",
            "--precondition", "--seed", "3", "--solution_dir", str(tmp_path / "sol")]
    assert main(args) == 0
    z = np.load(tmp_path / "sol" / "afiro.npz")
    res = tp.solve_lp(AFIRO, precondition=True, primal_weight_update=True, adaptive_stepsize=True, seed=3)
    for k in ("x", "y", "reduced_costs", "row_activity"):
        np.testing.assert_array_equal(z[k], getattr(res, k).cpu().numpy().reshape(-1))
    for k in ("objective", "dual_objective", "primal_residual", "dual_residual", "gap", "rel_primal_residual", "rel_dual_residual", "rel_gap"):
        assert float(z[k]) == getattr(res, k)
    assert str(z["status"]) == res.status == "Solved"
    header = open(tmp_path / "out" / "solver_results.csv").readline().strip().split(",")
    assert header == ["File", "Objective", "Iterations (k)", "Restarts (n)", "KKT Passes (j)", "Time (s)", "Status"]


# ---------------------------------------------------------------------------------------------------------------------------------
# sharded: two ranks share the card
# ---------------------------------------------------------------------------------------------------------------------------------
def _sharded_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        lp = tp.gen_lp(301, 403, 4, seed=21, recipe="mixed", ineq_frac=0.6, device=dev())
        problem = (lp.c, tp.CsrPair(lp.m, lp.n, lp.rowptr, lp.colidx, lp.val), lp.q, lp.m_ineq, lp.l, lp.u)
        kw = dict(tol=1e-4, primal_weight_update=True, adaptive_stepsize=True, seed=1)
        res = tp.solve_lp(problem, comm=True, **kw)
        assert res.status == "Solved"
        P, _ = original_problem(problem, torch.float32)
        u = np.finfo(np.float32).eps
        assert not check_result_against_the_original_problem(res, P, False, 1e-4, u)   # every rank: the full vectors, the whole sums
        if rank == 0:
            one = tp.solve_lp(problem, **kw)
            assert not check_result_against_the_original_problem(one, P, False, 1e-4, u)
            # the one-GPU report of the SAME point: the sharded result's x and y put into a one-GPU engine
            eng = tp.PdlpEngine.from_full(problem[1], lp.c, lp.q, lp.l, lp.u, lp.m_ineq)
            eng.set_iterate(res.x.view(-1), res.y.view(-1))
            rep = eng.report(N.CUR)
            x, y = h64(res.x), h64(res.y)
            lam, act, s, e_lam, e_act, b = ref_report(P, x, y, 0, u)
            assert_within(h64(res.reduced_costs), h64(rep["reduced_costs"]), 2 * e_lam, "sharded against one GPU: reduced costs")
            assert_within(h64(res.row_activity), h64(rep["row_activity"]), 2 * e_act, "sharded against one GPU: row activity")
            assert torch.equal(res.y.view(-1), rep["y"])
            assert_within(res.objective, rep["p"], 2 * (b[3] + u * abs(s[3])), "sharded against one GPU: objective")
            e_d = b[5] + b[1] + b[2] + 3 * u * (abs(s[5]) + abs(s[1]) + abs(s[2]))
            assert_within(res.dual_objective, rep["d_adj"], 2 * e_d, "sharded against one GPU: dual objective")
            for name, key, v, e in (("primal_residual", "pr", s[4], b[4]), ("dual_residual", "dr", s[0], b[0])):
                e_root = min(np.sqrt(C_BOUND * e), e / max(np.sqrt(v), 1e-300)) + u * np.sqrt(v)
                assert_within(getattr(res, name), rep[key], 2 * e_root, f"sharded against one GPU: {name}")
        ret[rank] = "ok"
    finally:
        dist.destroy_process_group()


def test_sharded_report_matches_one_gpu():
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with mp.Manager() as man:
        ret = man.dict()
        mp.spawn(_sharded_worker, args=(2, port, ret), nprocs=2, join=True)
        assert dict(ret) == {0: "ok", 1: "ok"}
