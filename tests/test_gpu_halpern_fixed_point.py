"""The fixed-point residual of the Halpern iteration on the GPU (pdlp_halpern_fixed_point, PdlpEngine.halpern_fixed_point,
solve_lp(halpern_restart="fixed_point")): the three sums of the pass against float64 numpy over the vectors the handle holds, within
the running-error bound of the kernel's own arithmetic, through every product form the epilogue is instantiated for (CSR row
blocks, column-sorted row blocks, long rows, tiles in one launch, tiles in panel groups, tiles with a remainder) in float32 and
float64; that the pass moves nothing else; the call-sequence rule; and whole solves, one of them against a float64 numpy model of
the whole driver restart by restart."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

import torchpdlp_amd as tp
from tests.halpern_fp_model import fixed_point_driver_model
from tests.host_lp import DEV, NP, HostLP, get_lp
from tests.quad_model import make_qp, model_of_qp
from tests.ranged_model import RangedModel, feasible_ranged_lp
from tests.test_gpu_batch_kernels import C_BOUND, U64
from tests.test_gpu_halpern import AFIRO, AFIRO_OPT, SCENARIOS, check_solution, host, put, start_points
from torchpdlp_amd import _native as N
from torchpdlp_amd import rules

DTYPES = [torch.float32, torch.float64]
STATE = "call sequence"
ITERATE_BUFFERS = (N.BUF_X_CUR, N.BUF_X_PREV, N.BUF_X_AVG, N.BUF_Y_CUR, N.BUF_Y_PREV, N.BUF_Y_AVG, N.BUF_XBAR, N.BUF_SCALARS,
                   N.BUF_X_SUM, N.BUF_Y_SUM)


@pytest.fixture(scope="module", autouse=True)
def _setup():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    N.load()


def dev(v, dtype):
    return torch.tensor(np.asarray(v), dtype=dtype, device=DEV)


def reference(A, eng):
    """the three sums in float64 numpy from PDLP_PREV (z) and PDLP_AVG (T(z)) as the handle holds them, and the bound of the
    kernel's arithmetic on each.  With u the unit roundoff of the working precision: d = fl(a - b) carries a relative u, so d^2 a
    relative 2u, and the double sum of `len` terms (len + 2) u64 of the terms' sizes.  A row of K' of length L over dy = fl(...)
    is off by (L + 1) u (|K'||dy|)_j plus u (|K'||dy|)_j for dy's own rounding; the product with dx = fl(...) adds u of its size --
    granted: (L_j + 2) u (|K'||dy|)_j |dx_j| per row, and (n + 2) u64 of the terms' sizes for the double sum."""
    u = float(np.finfo(NP[eng.dtype]).eps) / 2
    (zx, zy), (xc, yc) = ((host(v) for v in eng.get_iterate(w)) for w in (N.PREV, N.AVG))
    dx, dy = zx - xc, zy - yc
    KT = sp.csr_matrix(A.T)
    L = np.diff(KT.indptr)
    ktdy, mag = KT @ dy, abs(KT) @ np.abs(dy)
    m, n = A.shape
    dx2, dy2, cross = float(dx @ dx), float(dy @ dy), float(dx @ ktdy)
    bounds = (2 * u * dx2 + (n + 2) * U64 * dx2,
              float(np.sum((L + 2) * u * mag * np.abs(dx))) + (n + 2) * U64 * float(np.sum(np.abs(ktdy * dx))),
              2 * u * dy2 + (m + 2) * U64 * dy2)
    return (dx2, cross, dy2), bounds, (zx, zy, xc, yc)


def check_pass(A, eng, tag):
    got = eng.halpern_fixed_point()
    ref, bounds, pts = reference(A, eng)
    for name, g, r, b in zip(("dx2", "cross", "dy2"), got, ref, bounds):
        print(f"{tag} {name}: got {g!r} ref {r!r} |diff| {abs(g - r):.3e} bound {C_BOUND * b:.3e}")
        assert abs(g - r) <= C_BOUND * b, (tag, name, g, r, abs(g - r), C_BOUND * b)
    # the pass again gives the same bits (fixed summation order, no atomics), and dy went where the header says
    assert eng.halpern_fixed_point() == got
    assert np.array_equal(host(eng.buffer(N.BUF_DY)), host(dev(pts[1], eng.dtype) - dev(pts[3], eng.dtype)))
    return got, pts


# ---------------------------------------------------------------------------------------------------
# 1. the pass, in every form
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name,form", SCENARIOS, ids=[f"{a}-{b}" for a, b in SCENARIOS])
def test_pass_against_numpy(name, form, dtype):
    lp = get_lp(name)
    e = lp.engine(dtype, form)
    eta, omega = 0.9 / lp.norm2(), 0.8
    x0, y0, x1, y1 = start_points(lp, dtype)
    put(e, x0, y0, x1, y1, eta, omega)
    done = 0
    for upto in (1, 2, 41):
        zx, zy = (v.clone() for v in e.get_iterate(N.CUR))
        e.halpern_iterate(upto - done)
        if upto - done == 1:
            # one iteration in the call: PDLP_PREV is the iterate it started from, bit for bit
            px, py = e.get_iterate(N.PREV)
            assert torch.equal(px, zx) and torch.equal(py, zy)
        done = upto
        (dx2, cross, dy2), _ = check_pass(lp.A, e, f"{name}:{form}:{upto}")
        # the residual the driver forms from them is a number (the metric is positive definite for eta < 1 / ||K||)
        r = rules.fixed_point_error(dx2, cross, dy2, NP[dtype](eta), NP[dtype](omega))
        assert np.isfinite(r) and (r > 0 or (dx2 == 0 and dy2 == 0))


# ---------------------------------------------------------------------------------------------------
# 2. nothing else moves
# ---------------------------------------------------------------------------------------------------
def occurrences(ws: bytes, pattern: bytes):
    out, at = [], ws.find(pattern)
    while at >= 0:
        out.append(at)
        at = ws.find(pattern, at + 1)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name,form", [("mid", "tiles_groups"), ("long", "csr"), ("mid_dense", "tiles_remainder"), ("edge_free_and_fixed", "sorted")])
def test_pass_moves_nothing_else(name, form, dtype):
    lp = get_lp(name)
    eta, omega = 0.9 / lp.norm2(), 0.8
    pts = start_points(lp, dtype)
    e, plain = lp.engine(dtype, form), lp.engine(dtype, form)
    put(e, *pts, eta, omega)
    put(plain, *pts, eta, omega)
    e.halpern_iterate(7)
    plain.halpern_iterate(7)
    before = [e.buffer(b).clone() for b in ITERATE_BUFFERS]
    ptrs = [e.buffer(b).data_ptr() for b in ITERATE_BUFFERS]
    # x_last / y_last have no buffer id: they hold the anchor (x0, y0) of `put`, which no iterate buffer holds any more -- every place
    # of the workspace with those bytes
    ws = e.workspace.cpu().numpy().tobytes()
    last = [(at, p) for p in (pts[0].tobytes(), pts[1].tobytes()) for at in occurrences(ws, p)]
    assert {p for _, p in last} == {pts[0].tobytes(), pts[1].tobytes()}
    for _ in range(3):
        e.halpern_fixed_point()
    e.synchronize()
    assert [e.buffer(b).data_ptr() for b in ITERATE_BUFFERS] == ptrs                  # (no role moved)
    for b, was in zip(ITERATE_BUFFERS, before):
        now = e.buffer(b)
        assert torch.equal(now.view(torch.uint8), was.view(torch.uint8)), b           # (bits: the scalar block may hold anything)
    ws = e.workspace.cpu().numpy().tobytes()
    assert all(ws[at:at + len(p)] == p for at, p in last)
    # 40 further iterations, a KKT pass and a restart: the bits of the run without the pass
    for g in (e, plain):
        g.halpern_iterate(40)
    e.halpern_fixed_point()
    ka, kb = e.kkt(N.AVG, omega), plain.kkt(N.AVG, omega)
    assert ka == kb
    for g in (e, plain):
        g.restart(N.AVG)
        g.mark_restart_point()
        g.halpern_iterate(3)
    for w in (N.CUR, N.AVG, N.PREV):
        assert all(torch.equal(a, b) for a, b in zip(e.get_iterate(w), plain.get_iterate(w))), w
    assert torch.equal(e.buffer(N.BUF_XBAR), plain.buffer(N.BUF_XBAR))
    assert e.scalars() == plain.scalars()


# ---------------------------------------------------------------------------------------------------
# 3. with q_upper and quad_diag set: the pass reads vectors only
# ---------------------------------------------------------------------------------------------------
_QP = {}


def qp_lp():
    if not _QP:
        qp = make_qp(600, 520, 17, per_row=8)
        i = np.arange(qp.m)
        qu = np.full(qp.m, np.inf)
        two = (i < qp.m_ineq) & (i % 4 >= 2)
        qu[two] = qp.q[two] + 0.5
        _QP.update(qp=qp, qu=qu, lp=HostLP(qp.A, qp.m_ineq, qp.c, qp.q, qp.l, qp.u), mo=model_of_qp(qp, qu))
    return _QP["qp"], _QP["qu"], _QP["lp"], _QP["mo"]


@pytest.mark.parametrize("dtype,form", [(torch.float32, "tiles_groups"), (torch.float64, "sorted"), (torch.float32, "csr"), (torch.float64, "tiles")],
                         ids=["f32-tiles_groups", "f64-sorted", "f32-csr", "f64-tiles"])
def test_pass_with_two_sided_rows_and_quadratic_term(dtype, form):
    qp, qu, lp, mo = qp_lp()
    e = lp.engine(dtype, form, quad_diag=dev(qp.d, dtype), q_upper=dev(qu, dtype))
    assert e.quad_diag is not None and e.q_upper is not None
    eta, omega = 0.9 / lp.norm2(), 0.8
    T = NP[dtype]
    tau, sigma = float(T(eta) / T(omega)), float(T(eta) * T(omega))
    x0, y0, x1, y1 = start_points(lp, dtype)
    put(e, x0, y0, x1, y1, eta, omega)
    done = 0
    for upto in (1, 2, 41):
        e.halpern_iterate(upto - done)
        done = upto
        _, (zx, zy, xc, yc) = check_pass(lp.A, e, f"qp:{form}:{upto}")
        # PDLP_AVG is one step of the two-sided, quadratic operator from PDLP_PREV (the model's step, within what
        # tests/test_gpu_halpern.py grants a model comparison in this precision)
        mxc, myc, _, _ = mo.step(zx, zy, tau, sigma)
        tol = 3e-5 if dtype == torch.float32 else 1e-11
        np.testing.assert_allclose(xc, mxc, rtol=tol, atol=tol * max(1.0, float(np.abs(mxc).max())))
        np.testing.assert_allclose(yc, myc, rtol=tol, atol=tol * max(1.0, float(np.abs(myc).max())))
    assert (np.abs(yc[:qp.m_ineq]) > 0).any() and (yc[:qp.m_ineq] < 0).any()         # (upper sides are in play)


# ---------------------------------------------------------------------------------------------------
# 4. call sequence
# ---------------------------------------------------------------------------------------------------
def test_call_sequence():
    lp = get_lp("edge_free_and_fixed")
    dtype = torch.float32
    x0, y0, x1, y1 = start_points(lp, dtype)
    e = lp.engine(dtype)
    refused = lambda g=e: pytest.raises(N.PdlpError, match=STATE)
    # a new handle, and one with an iterate but no Halpern iteration
    with refused():
        e.halpern_fixed_point()
    put(e, x0, y0, x1, y1, 0.1, 0.8)
    with refused():
        e.halpern_fixed_point()
    e.halpern_iterate(0)                                   # (no iteration: nothing to evaluate)
    with refused():
        e.halpern_fixed_point()
    e.halpern_iterate(2)
    first = e.halpern_fixed_point()
    # KKT, report and distance passes leave the pair where it is
    e.kkt(N.AVG, 0.8)
    e.kkt(N.CUR, 0.8)
    e.report(N.AVG)
    e.restart_distance()
    e.set_omega(0.7)
    assert e.halpern_fixed_point() == first
    # right after a restart (at the candidate or at the current iterate) and after set_iterate
    e.restart(N.AVG)
    with refused():
        e.halpern_fixed_point()
    e.mark_restart_point()
    with refused():
        e.halpern_fixed_point()
    e.halpern_iterate(1)
    e.halpern_fixed_point()
    e.restart(N.CUR)
    with refused():
        e.halpern_fixed_point()
    e.halpern_iterate(1)
    e.halpern_fixed_point()
    e.set_iterate(dev(x0, dtype), dev(y0, dtype))
    with refused():
        e.halpern_fixed_point()
    # after a PDHG iterate, fixed or adaptive, and after the half-step calls
    e.halpern_iterate(3)
    e.halpern_fixed_point()
    e.iterate(1, False)
    with refused():
        e.halpern_fixed_point()
    e.halpern_iterate(1)
    e.halpern_fixed_point()
    e.iterate(2, True)
    with refused():
        e.halpern_fixed_point()
    e.halpern_iterate(1)
    e.halpern_fixed_point()
    N.check(e.lib.pdlp_primal_half(e.h, 0), "pdlp_primal_half")
    with refused():
        e.halpern_fixed_point()
    N.check(e.lib.pdlp_dual_half(e.h, 0), "pdlp_dual_half")
    with refused():
        e.halpern_fixed_point()
    e.halpern_iterate(1)
    e.halpern_fixed_point()
    # the handles pdlp_halpern_iterate refuses: mixed precision (in delta mode or not), graph replay switched on
    for delta in (True, False):
        em = lp.engine(torch.float32, vec_dtype=torch.float64, delta=delta)
        em.set_iterate(dev(x0, torch.float64), dev(y0, torch.float64))
        with pytest.raises(N.PdlpError, match=STATE):
            em.halpern_fixed_point()
    e.set_option(N.OPT_GRAPH, 1)
    with refused():
        e.halpern_fixed_point()
    e.set_option(N.OPT_GRAPH, 0)
    e.halpern_fixed_point()


# ---------------------------------------------------------------------------------------------------
# 5. whole solves
# ---------------------------------------------------------------------------------------------------
SOLVES = {"f64_1e-8": (torch.float64, 1e-8), "f32_1e-4": (torch.float32, 1e-4)}


@pytest.mark.parametrize("mode", list(SOLVES))
def test_solve_lp_afiro(mode):
    dtype, tol = SOLVES[mode]
    trace = dict(kkt=[], omega=[], restarts=[])
    res = tp.solve_lp(AFIRO, tol=tol, halpern=True, halpern_restart="fixed_point", primal_weight_update=True, dtype=dtype, seed=3,
                      max_kkt=2_000_000, trace=trace)
    problem = tp.mps_to_standard_form(AFIRO, device=DEV, dtype=dtype)
    bound = 1e-3 * (1 + abs(AFIRO_OPT)) if tol == 1e-4 else 2e-8 * (1 + 2 * abs(AFIRO_OPT))
    check_solution(res, problem, tol, bound, AFIRO_OPT)
    print(f"afiro {mode}: fixed-point rule k={res.iterations} n={res.restarts} j={res.kkt_passes}")
    # the accounting: iterations + one evaluation per restart period (r0) and per check + two per restart
    k, n, j = res.iterations, res.restarts, res.kkt_passes
    assert k % 40 == 0 and j == k + n + k // 40 + 2 * n and len(trace["restarts"]) == n
    assert all(u == 1 and c in (0, 1, 2) and tt % 40 == 0 for c, tt, u in trace["restarts"])


def test_solve_lp_tiled_600x520(monkeypatch):
    """test_gpu_halpern.py's tiled LP (both products of the solve's engine on k_tiled_fused) under the fixed-point rule"""
    monkeypatch.setenv("PDLP_TILED", "1")
    monkeypatch.setenv("PDLP_TILE_LW", "6")
    lp = tp.gen_lp(600, 520, 8, seed=11, device=DEV, recipe="mixed")
    K = tp.CsrPair(lp.m, lp.n, lp.rowptr, lp.colidx, lp.val)
    problem = (lp.c, K, lp.q, lp.m_ineq, lp.l, lp.u)
    eng = tp.PdlpEngine.from_full(K, lp.c, lp.q, lp.l, lp.u, lp.m_ineq)
    assert all(k.startswith("tiled") for k in eng.kernels), eng.kernels
    del eng
    res = tp.solve_lp(problem, tol=1e-4, halpern=True, halpern_restart="fixed_point", primal_weight_update=True, seed=3, max_kkt=2_000_000)
    check_solution(res, problem, 1e-4, 1e-3 * (1 + abs(lp.opt_obj)), lp.opt_obj)
    print(f"600x520 tiled: fixed-point rule k={res.iterations} n={res.restarts} j={res.kkt_passes}")


MODEL_LP = dict(m=40, n=60, per_row=4, seed=2, tol=1e-6)


def test_solve_follows_the_model_restart_by_restart():
    """A float64 solve of a 40 x 60 LP with two-sided rows against the float64 numpy model of the whole driver
    (tests/halpern_fp_model.py): the same restarts (criterion, iterations since the last one) and the same iteration count.  Every
    threshold comparison of the model's run is further than a relative 1e-9 from flipping (asserted; this seed: 1.5e-4, with all
    three criteria in the list), where float64 rounding moves a residual by some 1e-13: a mismatch is a bug, not rounding."""
    A, m_ineq, c, q, l, u, qu = feasible_ranged_lp(MODEL_LP["m"], MODEL_LP["n"], MODEL_LP["per_row"], MODEL_LP["seed"])
    mo = RangedModel(A, m_ineq, c, q, l, u, qu)
    sigma = float(np.linalg.norm(mo.A, 2))
    ref = fixed_point_driver_model(mo, sigma, MODEL_LP["tol"], primal_update=True)
    assert ref["status"] == "Solved" and ref["margin"] > 1e-9, ref["margin"]
    assert {crit for crit, _, _ in ref["restarts"]} == {0, 1, 2}
    t = lambda v: dev(v, torch.float64)
    trace = dict(kkt=[], omega=[], restarts=[])
    x, obj, k, n, j, status, _ = tp.pdlp_algorithm(tp.CsrPair.from_any(A, device=DEV, dtype=torch.float64), m_ineq, t(c), t(q), t(l), t(u),
                                                   DEV, tol=MODEL_LP["tol"], verbose=False, primal_update=True, sigma=sigma, trace=trace,
                                                   halpern=True, halpern_restart="fixed_point", q_upper=t(qu), max_kkt=1_000_000)
    print(f"model LP: GPU k={k} n={n} j={j} restarts={trace['restarts']}; model k={ref['k']} n={ref['n']} j={ref['j']} margin={ref['margin']:.3e}")
    assert status == "Solved"
    assert [(cr, tt) for cr, tt, _ in trace["restarts"]] == [(cr, tt) for cr, tt, _ in ref["restarts"]]
    assert (k, n, j) == (ref["k"], ref["n"], ref["j"])
    np.testing.assert_allclose(host(x).reshape(-1), ref["x"], rtol=1e-9, atol=1e-9)


# ---------------------------------------------------------------------------------------------------
# 6. the default is unchanged
# ---------------------------------------------------------------------------------------------------
def test_default_is_the_kkt_rule():
    runs = []
    for kw in ({}, dict(halpern_restart="kkt")):
        trace = dict(kkt=[], omega=[], restarts=[])
        res = tp.solve_lp(AFIRO, tol=1e-4, halpern=True, primal_weight_update=True, dtype=torch.float32, seed=3, max_kkt=2_000_000,
                          trace=trace, **kw)
        assert res.status == "Solved"
        runs.append((res.x.cpu().numpy().tobytes(), res.objective, res.iterations, res.restarts, res.kkt_passes, trace))
    assert runs[0] == runs[1]
    # and it is not the fixed-point rule: the KKT rule makes one KKT pass per check, which its trace shows as a finite kkt_avg of a
    # candidate whose kkt_cur is inf, and counts no r0
    k, n, j = runs[0][2:5]
    assert j == k + k // 40 + 2 * n
