"""The reflected Halpern iteration on the GPU (pdlp_halpern_iterate, PdlpEngine.halpern_iterate, solve_lp(halpern=True)):
the candidate against the PDHG kernels bit for bit, the combination step element by element, six iterations against a float64
numpy model, the handle's state around the new call, and whole solves -- through every product form the epilogues are
instantiated for (CSR row blocks, column-sorted row blocks, long rows, tiles in one launch, tiles in panel groups, tiles with a
remainder), in float32 and float64, on small shapes."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as orc                                   # the checker (tests only)
import torchpdlp_amd as tp
from tests.conftest import GOLDEN
from tests.host_lp import DEV, NP, get_lp          # the LPs (float64 numpy on the host; every value is a float32 number)
from torchpdlp_amd import _native as N
from torchpdlp_amd.rules import halpern_weights

AFIRO = os.path.join(GOLDEN, "mps", "afiro.mps")
AFIRO_OPT = -464.7531428571
DTYPES = [torch.float32, torch.float64]
FORMS = ["csr", "sorted", "tiles", "tiles_groups", "tiles_remainder"]


@pytest.fixture(scope="module", autouse=True)
def _setup():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    orc.set_threads(1)
    N.load()


EDGE = ["edge_no_ineq", "edge_all_ineq", "edge_empty_row_and_col", "edge_one_by_one", "edge_free_and_fixed"]
# (LP, product form): 37 x 23 and 1 x 1 have one panel, so no panel groups and nothing for a remainder; 600 x 520 has several row
# blocks of K and of K' in every form (256-row CSR blocks, 512-row tile blocks) and 9 panels of 64 columns; the dense row and
# column of `mid_dense` put 64 > 15 items of one row into one tile (the remainder), and those of `long` (2300 and 2500 entries) are
# longer than the CSR kernel's 2048-entry block: k_long_rows runs the epilogue
SCENARIOS = ([(lp, f) for lp in EDGE for f in ("csr", "sorted", "tiles")] +
             [("mid", f) for f in ("csr", "sorted", "tiles", "tiles_groups")] + [("mid_dense", "tiles_remainder")] +
             [("long", f) for f in ("csr", "sorted", "tiles_remainder")])


def start_points(lp, dtype, seed=3):
    """an anchor and a DIFFERENT iterate, both random (the iterate need not respect the bounds: a Halpern iterate does not)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.where(np.isinf(lp.l), -3, lp.l), np.where(np.isinf(lp.u), 3, lp.u)
    x0 = np.clip(rng.standard_normal(lp.n), lo, hi)
    y0 = rng.standard_normal(lp.m)
    y0[:lp.m_ineq] = np.abs(y0[:lp.m_ineq])
    x1, y1 = x0 + 0.3 * rng.standard_normal(lp.n), y0 + 0.3 * rng.standard_normal(lp.m)
    return [v.astype(NP[dtype]) for v in (x0, y0, x1, y1)]


def put(eng, x0, y0, x1, y1, eta, omega):
    """anchor (x0, y0), iterate (x1, y1), t = 0: set_iterate at the anchor, then the iterate written through the buffer views (a
    restart-free path: nothing of the handle's state changes)"""
    t = lambda v: torch.tensor(v, dtype=eng.dtype, device=DEV)
    eng.set_iterate(t(x0), t(y0))
    eng.set_step(float(eta), float(omega), 1.0, 0)
    eng.buffer(N.BUF_X_CUR)[:] = t(x1)
    eng.buffer(N.BUF_Y_CUR)[:] = t(y1)


def model_step(lp, x, y, xa, ya, t, tau, sigma):
    """one iteration of the method in float64 with dense products -> (x+, y+, x', y', xbar)"""
    a, b = (t + 1) / (t + 2), 1 / (t + 2)
    xc = np.clip(x - tau * (lp.c - lp.A.T @ y), lp.l, lp.u)
    xbar = xc + (xc - x)
    yc = y + sigma * (lp.q - lp.A @ xbar)
    yc[:lp.m_ineq] = np.maximum(yc[:lp.m_ineq], 0)
    return a * xbar + b * xa, a * (2 * yc - y) + b * ya, xc, yc, xbar


def close(got, ref, tol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * max(1.0, float(np.max(np.abs(ref))) if ref.size else 1.0))


def host(v):
    return v.detach().cpu().numpy().astype(np.float64)


def check_combination(eng, it, z_before, anchor):
    """x+ = a xbar + b x_last and y+ = a (2y' - y) + b y_last element by element, from what the handle holds after the iteration.
    Bound: a and b are exact inputs (already rounded).  With u = eps/2, fl(a xbar) and fl(b x_last) each carry a relative u and
    their sum another u: |error| <= u (|a xbar| + |b x_last|) + u |x+| <= eps (|a xbar| + |b x_last|) to first order.  For y the
    reflected point w = fl(2y' - y) adds one more rounding (2y' is exact), u |w| <= u (2|y'| + |y|), scaled by a:
    |error| <= eps (a (2|y'| + |y|) + |b y_last|) + u a (2|y'| + |y|).  Granted: 2 eps times the sum of the magnitudes of the
    terms, plus the smallest normal number for a product that underflows."""
    T = NP[eng.dtype]
    a, b = (float(v) for v in halpern_weights(it, eng.dtype))
    eps, tiny = float(np.finfo(T).eps), float(np.finfo(T).tiny)
    (x, y), (xl, yl) = z_before, anchor
    xn, yn = (host(v) for v in eng.get_iterate(N.CUR))
    xc, yc = (host(v) for v in eng.get_iterate(N.AVG))
    xbar = host(eng.buffer(N.BUF_XBAR))
    ex = np.abs(xn - (a * xbar + b * xl))
    bx = 2 * eps * (np.abs(a * xbar) + np.abs(b * xl)) + tiny
    assert (ex <= bx).all(), (it, float((ex / bx).max()))
    ey = np.abs(yn - (a * (2 * yc - y) + b * yl))
    by = 2 * eps * (a * (2 * np.abs(yc) + np.abs(y)) + np.abs(b * yl)) + tiny
    assert (ey <= by).all(), (it, float((ey / by).max()))
    return xc, yc


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name,form", SCENARIOS, ids=[f"{a}-{b}" for a, b in SCENARIOS])
def test_halpern_iterations(name, form, dtype):
    """checks 1 to 4 of one (LP, product form, precision): see the comments at each"""
    lp = get_lp(name)
    e, p = lp.engine(dtype, form), lp.engine(dtype, form)          # p: the PDHG kernels on the same form
    eta, omega = 0.9 / lp.norm2(), 0.8
    T = NP[dtype]
    tau, sigma = float(T(eta) / T(omega)), float(T(eta) * T(omega))         # (as k_set_step rounds them)
    x0, y0, x1, y1 = start_points(lp, dtype)
    put(e, x0, y0, x1, y1, eta, omega)
    mx, my, ma = x1.astype(np.float64), y1.astype(np.float64), (x0.astype(np.float64), y0.astype(np.float64))
    for it in range(6):
        zx, zy = e.get_iterate(N.CUR)
        e.halpern_iterate(1)
        xc, yc = e.get_iterate(N.AVG)
        # 1. the candidate and xbar equal one fixed PDHG step of the parent's kernels from z, bit for bit (t = 0 and t = 5 asked;
        #    every t is as cheap)
        p.set_iterate(zx, zy)
        p.set_step(float(eta), float(omega), 1.0, 0)
        p.iterate(1, False)
        px, py = p.get_iterate(N.CUR)
        assert torch.equal(px, xc) and torch.equal(py, yc), it
        assert torch.equal(p.buffer(N.BUF_XBAR), e.buffer(N.BUF_XBAR)), it
        # 2. the combination with t = it (a stale or wrong t shows at it = 1 and 5) and the anchor of set_iterate
        xch, ych = check_combination(e, it, (host(zx), host(zy)), ma)
        assert (xch >= lp.l).all() and (xch <= lp.u).all() and (ych[:lp.m_ineq] >= 0).all()
        mx, my, mxc, myc, _ = model_step(lp, mx, my, ma[0], ma[1], it, tau, sigma)
    # 3. six iterations against the float64 model: float32 within what test_edge_cases_match_oracle grants six PDHG steps; float64
    #    1e-11 max|ref| (a few hundred roundings of 1.1e-16 per entry on O(10) data; the operator is non-expansive)
    tol = 3e-5 if dtype == torch.float32 else 1e-11
    xg, yg = e.get_iterate(N.CUR)
    close(host(xg), mx, tol)
    close(host(yg), my, tol)
    close(host(xc), mxc, tol)
    close(host(yc), myc, tol)
    # 4. state.  The KKT pass at the candidate multiplies (nothing of the running sums): the oracle's numbers at the same point
    got, ref = e.kkt(N.AVG, omega), lp.oracle(dtype).kkt(xc.cpu().numpy(), yc.cpu().numpy(), omega)
    for key in ("pr", "dr", "gap", "p", "d_adj", "kkt"):
        np.testing.assert_allclose(got[key], float(ref[key]), rtol=1e-4, atol=2e-5, err_msg=f"{name}:{form}:{key}")
    final = [v.clone() for v in (xg, yg, xc, yc)]
    # ... a report and KKT passes between two calls change no later bit; neither does the grouping of the iterations into calls
    put(e, x0, y0, x1, y1, eta, omega)
    e.halpern_iterate(3)
    e.report(N.CUR)
    e.report(N.AVG)
    e.kkt(N.AVG, omega)
    e.kkt(N.CUR, omega)
    e.halpern_iterate(3)
    again = list(e.get_iterate(N.CUR)) + list(e.get_iterate(N.AVG))
    assert all(torch.equal(a, b) for a, b in zip(again, final))
    # ... and a second handle (which has iterated with PDHG before: set_iterate wipes that) gives the same bits in one call
    put(p, x0, y0, x1, y1, eta, omega)
    p.halpern_iterate(6)
    other = list(p.get_iterate(N.CUR)) + list(p.get_iterate(N.AVG))
    assert all(torch.equal(a, b) for a, b in zip(other, final))
    # after a restart at the candidate and the mark, the next iteration runs with t = 0 from the new anchor
    e.restart(N.AVG)
    e.mark_restart_point()
    zx, zy = e.get_iterate(N.CUR)
    assert torch.equal(zx, final[2]) and torch.equal(zy, final[3])
    e.halpern_iterate(1)
    check_combination(e, 0, (host(zx), host(zy)), (host(zx), host(zy)))
    mx, my, _, _, _ = model_step(lp, mxc, myc, mxc, myc, 0, tau, sigma)
    xg, yg = e.get_iterate(N.CUR)
    close(host(xg), mx, tol)
    close(host(yg), my, tol)


def test_calls_that_have_no_halpern_form_are_refused():
    lp = get_lp("edge_free_and_fixed")
    x0, y0, x1, y1 = start_points(lp, torch.float32)
    # a mixed-precision handle, in delta mode or not
    for delta in (True, False):
        em = lp.engine(torch.float32, vec_dtype=torch.float64, delta=delta)
        em.set_iterate(torch.tensor(x0, device=DEV), torch.tensor(y0, device=DEV))
        with pytest.raises(N.PdlpError, match="call sequence"):
            em.halpern_iterate(1)
    # graph replay switched on
    e = lp.engine(torch.float32)
    put(e, x0, y0, x1, y1, 0.1, 0.8)
    e.set_option(N.OPT_GRAPH, 1)
    with pytest.raises(N.PdlpError, match="call sequence"):
        e.halpern_iterate(1)
    e.set_option(N.OPT_GRAPH, 0)
    with pytest.raises(N.PdlpError, match="invalid"):
        e.halpern_iterate(-1)
    # the averaging calls would overwrite the candidate: refused from the first Halpern iteration to the next set_iterate
    e.halpern_iterate(2)
    cand = [v.clone() for v in e.get_iterate(N.AVG)]
    for call in (lambda: e.compute_average(), lambda: e.flush_average(False), lambda: e.flush_average(True)):
        with pytest.raises(N.PdlpError, match="call sequence"):
            call()
    e.kkt(N.AVG, 0.8)
    e.restart(N.AVG)
    with pytest.raises(N.PdlpError, match="call sequence"):
        e.compute_average()
    assert all(torch.equal(a, b) for a, b in zip(e.get_iterate(N.CUR), cand))
    put(e, x0, y0, x1, y1, 0.1, 0.8)
    e.iterate(3, False)
    e.kkt(N.CUR, 0.8)
    e.flush_average(False)
    e.compute_average()


# ---------------------------------------------------------------------------------------------------
# 5. whole solves
# ---------------------------------------------------------------------------------------------------
def check_solution(res, problem, tol, bound, opt, rel=True):
    c, K, q, m_ineq, l, u = problem
    assert res.status == "Solved", (res.status, res.iterations)
    assert abs(res.objective - opt) <= bound, (res.objective, opt)
    if rel:
        assert max(res.rel_primal_residual, res.rel_dual_residual, res.rel_gap) <= tol, \
            (res.rel_primal_residual, res.rel_dual_residual, res.rel_gap)
    x = res.x.view(-1)
    assert bool((x >= l.view(-1)).all()) and bool((x <= u.view(-1)).all())
    assert abs(float((c.view(-1).double() * x.double()).sum()) - res.objective) <= 1e-2


SOLVES = {"f32_1e-4": (torch.float32, 1e-4, {}), "f64_1e-8": (torch.float64, 1e-8, {}),
          "f32_1e-4_ruiz_pc": (torch.float32, 1e-4, dict(precondition=True, pock_chambolle=True))}


@pytest.mark.parametrize("mode", list(SOLVES))
def test_solve_lp_afiro(mode):
    dtype, tol, kw = SOLVES[mode]
    res = tp.solve_lp(AFIRO, tol=tol, halpern=True, primal_weight_update=True, dtype=dtype, seed=3, max_kkt=2_000_000, **kw)
    problem = tp.mps_to_standard_form(AFIRO, device=DEV, dtype=dtype)
    bound = 1e-3 * (1 + abs(AFIRO_OPT)) if tol == 1e-4 else 2e-8 * (1 + 2 * abs(AFIRO_OPT))
    if kw:      # (un-scaled x: inside the bounds up to the rounding of D_col * (l / D_col))
        c, K, q, m_ineq, l, u = problem
        eps = 4 * float(np.finfo(NP[dtype]).eps)
        problem = (c, K, q, m_ineq, l - eps * l.abs(), u + eps * u.abs())
    check_solution(res, problem, tol, bound, AFIRO_OPT, rel=not kw)
    print(f"afiro {mode}: halpern k={res.iterations} n={res.restarts} j={res.kkt_passes}")
    if mode == "f64_1e-8":
        # no more iterations than averaged PDHG with the same fixed step and the same seed (the host model: 0.53-0.65x)
        ref = tp.solve_lp(AFIRO, tol=tol, primal_weight_update=True, adaptive_stepsize=False, dtype=dtype, seed=3, max_kkt=2_000_000)
        print(f"afiro {mode}: averaged fixed-step PDHG k={ref.iterations} n={ref.restarts} j={ref.kkt_passes}")
        assert ref.status == "Solved"
        assert res.iterations <= ref.iterations, (res.iterations, ref.iterations)


def test_solve_lp_tiled_600x520(monkeypatch):
    """a tiled LP with a known optimum, all four bound classes: PDLP_TILED=1 with 64-column panels puts both products of the solve's
    engine on k_tiled_fused"""
    monkeypatch.setenv("PDLP_TILED", "1")
    monkeypatch.setenv("PDLP_TILE_LW", "6")
    lp = tp.gen_lp(600, 520, 8, seed=11, device=DEV, recipe="mixed")
    K = tp.CsrPair(lp.m, lp.n, lp.rowptr, lp.colidx, lp.val)
    problem = (lp.c, K, lp.q, lp.m_ineq, lp.l, lp.u)
    eng = tp.PdlpEngine.from_full(K, lp.c, lp.q, lp.l, lp.u, lp.m_ineq)
    assert all(k.startswith("tiled") for k in eng.kernels), eng.kernels
    del eng
    res = tp.solve_lp(problem, tol=1e-4, halpern=True, primal_weight_update=True, seed=3, max_kkt=2_000_000)
    check_solution(res, problem, 1e-4, 1e-3 * (1 + abs(lp.opt_obj)), lp.opt_obj)
    print(f"600x520 tiled: halpern k={res.iterations} n={res.restarts} j={res.kkt_passes}")
