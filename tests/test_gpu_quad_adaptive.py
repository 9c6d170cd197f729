"""The adaptive step of the sparse quadratic objective on the GPU (pdlp_objective_iterate, PdlpEngine.objective_iterate,
solve_lp(quad_step="adaptive")): six iterations call by call against the float64 model of tests/qp_adaptive_model.py with the
curvature inside its forward bound, a rejection that only the curvature term forces, the bit identities of the carried gradient,
whole solves of the table in DESIGN.md 4.5.1, and the refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import torchpdlp_amd as tp
from tests.host_lp import DEV, NP
from tests.qp_adaptive_model import adaptive_model_of
from tests.qp_model import make_general_qp
from tests.test_gpu_quad_matrix import begin, close, dev, gradient, host, lp_of, start_point, steps_of, tols
from tests.test_quad_adaptive_host import TABLE
from tests.test_quad_matrix_host import bound_of
from torchpdlp_amd import _native as N
from torchpdlp_amd.rules import qp_eta

DTYPES = [torch.float32, torch.float64]
DT_IDS = ["f32", "f64"]
INF = float("inf")
LD = np.longdouble
_QPS = {}


@pytest.fixture(scope="module", autouse=True)
def _setup():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert np.finfo(LD).eps < 1e-18, "the references of the float64 sums are formed in extended precision"
    N.load()


def qp_of(m, n, per_row, kind, seed=1, diag=False):
    """built once, shared, never written to"""
    key = (m, n, per_row, kind, seed, diag)
    if key not in _QPS:
        _QPS[key] = make_general_qp(m, n, seed, per_row, kind, diag=diag)
    return _QPS[key]


def coo(M):
    M = M.tocoo()
    return M.row, M.col, M.data.astype(LD)


def sums_at(qp, xo, yo, xn, yn):
    """the rule's four sums at the device's own step (xo, yo) -> (xn, yn), in extended precision"""
    dx, dy = (xn - xo).astype(LD), (yn - yo).astype(LD)
    ar, ac, av = coo(qp.A)
    qr, qc, qv = coo(qp.Q)
    return [float(np.sum(dx * dx)), float(np.sum(dy * dy)), float(np.sum(dy[ar] * av * dx[ac])), float(np.sum(dx[qr] * qv * dx[qc]))]


INSTANCES = {"37x23-seed1": (37, 23, None, "lowrank", 1), "37x23-seed2": (37, 23, None, "lowrank", 2),
             "600x520": (600, 520, 8, "sparse", 1), "300x2600": (300, 2600, 6, "arrow", 1)}


# ---------------------------------------------------------------------------------------------------
# 1. six iterations, call by call
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", list(INSTANCES))
def test_six_iterations_call_by_call_against_the_model(case, dtype):
    """x, y, g, eta and the verdict against the model's own run (the tolerances of tests/test_gpu_quad_matrix.py's six iterations);
    the four sums against extended-precision sums over the DEVICE's own step, each inside a forward bound of its rounding:
      ||dx||^2, ||dy||^2   d = v - x_old is rounded to T once and squared in double: 2 eps
      dy'K dx              K dx = (K xbar - K x) / (1 + theta) in T from a K x carried along (one rounding per iteration so far) and a
                           product of rowlen terms: eps sum_i |dy_i| (rowlen_i + 4 + 2 k) ((|K||xbar|)_i + (|K||x|)_i)
      dx'Q dx              DESIGN.md 4.5.1's bound, eps sum_j |dx_j| (|g'_j| + |g_j| + (|Q||x'|)_j rowlen_j)
    with eps the machine epsilon of the working type; the first three also get the worst case of their own addition in double,
    (number of terms) 2^-53 sum |term|, which only shows in float64"""
    m, n, per_row, kind, seed = INSTANCES[case]
    qp = qp_of(m, n, per_row, kind, seed)
    lp, mo = lp_of(qp), adaptive_model_of(qp)
    rtol, atol = tols(dtype)
    eps = float(np.finfo(NP[dtype]).eps)
    if case == "600x520":
        assert (np.diff(qp.Q.indptr) == 0).sum() > 20                       # (empty rows of Q: g_j = c_j, no curvature from them)
    if case == "300x2600":
        assert int(np.diff(qp.Q.indptr).max()) > 2048                       # (row 0 runs the long-row chunks)
    eta, omega, _, _ = steps_of(lp, qp.Q, dtype)
    x0, y0 = start_point(qp, dtype)
    e = lp.engine(dtype, quad_matrix=qp.Q)
    begin(e, x0, y0, eta, omega)
    absA, absQ = abs(qp.A), abs(qp.Q)
    lenA, lenQ = np.diff(qp.A.indptr), np.diff(qp.Q.indptr)
    mx, my, me = x0, y0, float(eta)
    for k in range(1, 7):
        xo, yo = (host(v) for v in e.get_iterate(N.CUR))
        eta_in = e.scalars()["eta"]
        e.objective_iterate(1)
        r = mo.rule(mx, my, me, omega, k)
        tag = f"{case}:{k}"
        xn, yn = (host(v) for v in e.get_iterate(N.CUR))
        xp, yp = (host(v) for v in e.get_iterate(N.PREV))
        assert np.array_equal(xp, xo) and np.array_equal(yp, yo), tag
        close(xn, r.x, dtype, tag + ":x")
        close(yn, r.y, dtype, tag + ":y")
        close(host(gradient(e)), r.g_new, dtype, tag + ":g")
        sc = e.scalars()
        red = host(e.buffer(N.BUF_RED))[:4]
        print(f"{tag} eta {sc['eta']:.9g} (model {r.eta_next:.9g}) eta_bar {sc['eta_bar']:.9g} ({r.eta_bar:.9g}) accepted {sc['accepted']:g} "
              f"({r.accepted}) curvature {sc['curvature']:.9g} ({r.curv:.9g}) 2dy'Kdx {sc['denominator']:.9g} ({r.den:.9g})")
        close([sc["eta"]], [r.eta_next], dtype, tag + ":eta")
        if abs(me - r.eta_bar) > 1e-3 * me:                                 # (the verdict is a comparison with eta_bar)
            assert bool(sc["accepted"]) == r.accepted, tag
        assert sc["k"] == k and sc["w_pending"] == (eta_in if sc["accepted"] else sc["eta"]), tag      # (step.py:110-115)
        assert sc["curvature"] == float(NP[dtype](red[3])) and sc["denominator"] == float(NP[dtype](2) * NP[dtype](red[2])), tag
        # the sums at the device's own step
        ref = sums_at(qp, xo, yo, xn, yn)
        xbar = xn + (xn - xo)
        add = 2.0 ** -53
        bounds = [(2 * eps + n * add) * ref[0], (2 * eps + m * add) * ref[1],
                  eps * float(np.abs(yn - yo) @ ((lenA + 4 + 2 * k) * (absA @ np.abs(xbar) + absA @ np.abs(xo))))
                  + m * add * float(np.abs(yn - yo) @ np.abs(qp.A @ (xn - xo))),
                  eps * float(np.abs(xn - xo) @ (np.abs(mo.grad(xn)) + np.abs(mo.grad(xo)) + (absQ @ np.abs(xn)) * lenQ))]
        for i, name in enumerate(("dx2", "dy2", "dyKdx", "dxQdx")):
            print(f"    {name}: device {red[i]:.17g} reference {ref[i]:.17g} error {abs(red[i] - ref[i]):.3g} bound {bounds[i]:.3g}")
            assert abs(red[i] - ref[i]) <= bounds[i], (tag, name, red[i], ref[i], bounds[i])
        assert ref[3] > 0 and bounds[3] < 0.1 * ref[3], tag                 # (the bound says something: the curvature is measured)
        assert abs(ref[3] - r.curv) <= 100 * rtol * abs(r.curv), tag        # (and it is the model's, at the model's step)
        mx, my, me = r.x, r.y, r.eta_next
    assert abs(me - eta) > 0.05 * eta                                       # (the rule has moved the step away from the start step)


# ---------------------------------------------------------------------------------------------------
# 2. a rejection that only the curvature forces
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", ["37x23-seed1", "600x520"])
def test_a_step_that_only_the_curvature_rejects(case, dtype):
    """two iterations in, at the primal weight 2^-10 (dx ~ eta / omega is long, dy ~ eta omega short: dx'Q dx outweighs 2 |dy'K dx|) and
    with eta = 50 x the model's eta_bar of that point: the LP's rule accepts the trial by a factor above 1.5, the full rule rejects
    it by a factor above 20 -- asserted on the model first.  The device reports the rejection, shrinks eta to the model's eta' and
    keeps the trial.  Fails on a build that drops the curvature term."""
    m, n, per_row, kind, seed = INSTANCES[case]
    qp = qp_of(m, n, per_row, kind, seed)
    lp, mo = lp_of(qp), adaptive_model_of(qp)
    T = NP[dtype]
    eta, omega, _, _ = steps_of(lp, qp.Q, dtype)
    x0, y0 = start_point(qp, dtype)
    e = lp.engine(dtype, quad_matrix=qp.Q)
    begin(e, x0, y0, eta, omega)
    e.objective_iterate(2)
    x, y = (host(v) for v in e.get_iterate(N.CUR))
    small = 2.0 ** -10
    L = float(np.linalg.norm(qp.Q.toarray(), 2))
    probe = mo.rule(x, y, float(qp_eta(lp.norm2(), L, small, T)), small, 3)
    big = float(T(50 * probe.eta_bar))
    full, lin = mo.rule(x, y, big, small, 3), mo.rule(x, y, big, small, 3, curvature=False)
    print(f"{case}: eta {big:.6g}; eta_bar with the curvature {full.eta_bar:.6g}, without {lin.eta_bar:.6g}; curvature {full.curv:.6g}, "
          f"2 dy'K dx {full.den:.6g}")
    assert lin.accepted and lin.eta_bar > 1.5 * big                          # the LP's bound would let the step through ...
    assert not full.accepted and 20 * full.eta_bar < big                     # ... the measured curvature does not
    assert np.array_equal(full.x, lin.x) and full.eta_next < 0.1 * big < lin.eta_next
    e.set_step(big, small, 1.0, 2)
    e.objective_iterate(1)
    sc = e.scalars()
    print(f"    device: accepted {sc['accepted']:g} eta {sc['eta']:.6g} (model {full.eta_next:.6g}) eta_bar {sc['eta_bar']:.6g} "
          f"curvature {sc['curvature']:.6g} 2 dy'K dx {sc['denominator']:.6g}")
    assert sc["accepted"] == 0 and sc["k"] == 3
    close([sc["eta"]], [full.eta_next], dtype, "the shrunk eta")
    close([sc["eta_bar"]], [full.eta_bar], dtype, "eta_bar")
    assert sc["w_pending"] == sc["eta"]                                      # (a rejected trial weighs with the shrunk step, step.py:113-115)
    xn, yn = (host(v) for v in e.get_iterate(N.CUR))
    rtol, atol = tols(dtype)
    scale = max(1.0, float(np.abs(full.x).max()))                            # (the long step moves free variables by hundreds)
    np.testing.assert_allclose(xn, full.x, rtol=rtol, atol=atol * scale, err_msg="the trial is kept: x")
    np.testing.assert_allclose(yn, full.y, rtol=rtol, atol=atol * scale, err_msg="the trial is kept: y")
    assert np.abs(xn - x).max() > 1.0
    xp, _ = e.get_iterate(N.PREV)
    assert np.array_equal(host(xp), x)


# ---------------------------------------------------------------------------------------------------
# 3. bit identities
# ---------------------------------------------------------------------------------------------------
SCALARS = ("eta", "omega", "tau", "sigma", "w_pending", "eta_sum", "k", "accepted", "eta_bar", "denominator")
FIXED_SCALARS = ("eta", "omega", "tau", "sigma", "eta_sum", "k")            # (what the fixed step writes)


def state(e, scalars=SCALARS):
    sc = e.scalars()
    return ([v.clone() for v in e.get_iterate(N.CUR)] + [e.buffer(b).clone() for b in (N.BUF_XBAR, N.BUF_X_SUM, N.BUF_Y_SUM)],
            {k: sc[k] for k in scalars})


def same(a, b):
    return len(a[0]) == len(b[0]) and all(torch.equal(u, v) for u, v in zip(a[0], b[0])) and a[1] == b[1]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_a_matrix_without_entries_is_the_adaptive_lp_bit_for_bit(dtype):
    """objective_iterate over a Q without stored entries against iterate(n, True) of an engine that never heard of Q: 12 iterations
    with a restart check and a restart to the average after 5, iterates, sums and scalars"""
    import scipy.sparse as sp
    qp = qp_of(600, 520, 8, "sparse")
    lp = lp_of(qp, scaled=True)
    eta, omega, _, _ = steps_of(lp, None, dtype)
    x0, y0 = start_point(qp, dtype)
    plain, zero = lp.engine(dtype), lp.engine(dtype, quad_matrix=sp.csr_matrix((qp.n, qp.n)))
    assert plain.quad_matrix is None and zero.quad_matrix is not None and zero.quad_matrix.nnz == 0
    outs = []
    for e, go in ((plain, lambda k: plain.iterate(k, True)), (zero, zero.objective_iterate)):
        out = []
        begin(e, x0, y0, eta, omega)
        for k in (1, 4):
            go(k)
            out.append(state(e))
        out.append(e.kkt(N.CUR, omega))
        e.flush_average(True)
        e.compute_average()
        out.append([v.clone() for v in e.get_iterate(N.AVG)])
        out.append(e.kkt(N.AVG, omega))
        e.restart(N.AVG)
        e.set_omega(0.5 * omega)
        e.mark_restart_point()
        for k in (1, 6):
            go(k)
            out.append(state(e))
        out.append(e.kkt(N.CUR, omega, unscaled=True))
        outs.append(out)
    a, b = outs
    assert a[0][1]["k"] == 1 and a[-2][1]["k"] == 12 and a[-2][1]["eta"] != eta
    for i, (u, v) in enumerate(zip(a, b)):
        if isinstance(u, dict):
            assert u == v, i
        elif isinstance(u, tuple):
            assert same(u, v), (i, u[1], v[1])
        else:
            assert all(torch.equal(p, q) for p, q in zip(u, v)), i
    assert zero.scalars()["curvature"] == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_the_carried_gradient_changes_no_bit(dtype):
    """objective_iterate(3) against three calls of objective_iterate(1); a KKT pass between two iterations -- at the previous iterate,
    which leaves g of ANOTHER point in the buffer, and at the current one, whose kept K'y the next half-step reads -- against the
    uninterrupted run; the fixed step on the same handle before and after against a fresh handle"""
    qp = qp_of(600, 520, 8, "sparse")
    lp = lp_of(qp)
    eta, omega, _, _ = steps_of(lp, qp.Q, dtype)
    x0, y0 = start_point(qp, dtype)
    more = SCALARS + ("curvature",)
    e, f = lp.engine(dtype, quad_matrix=qp.Q), lp.engine(dtype, quad_matrix=qp.Q)

    def full(eng):
        return state(eng, more), gradient(eng), eng.buffer(N.BUF_RED)[:4].clone()

    def same_full(a, b):
        return same(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    # one call of three against three calls of one
    begin(e, x0, y0, eta, omega)
    e.objective_iterate(3)
    begin(f, x0, y0, eta, omega)
    for _ in range(3):
        f.objective_iterate(1)
    three = full(e)
    assert same_full(three, full(f)) and three[0][1]["k"] == 3 and three[0][1]["curvature"] > 0
    e.objective_iterate(2)
    five = full(e)
    # a KKT pass at the PREVIOUS iterate in between: it forms g of that point; the next iteration forms its own again
    begin(f, x0, y0, eta, omega)
    f.objective_iterate(3)
    f.kkt(N.PREV, omega)
    assert not torch.equal(gradient(f), three[1])
    f.objective_iterate(2)
    assert same_full(five, full(f))
    # ... and a report, and a pass at the average
    begin(f, x0, y0, eta, omega)
    f.objective_iterate(3)
    f.report(N.PREV, omega=omega)
    f.objective_iterate(2)
    assert same_full(five, full(f))
    # a KKT pass at the CURRENT iterate keeps K'y: the next half-step is a vector pass over it, whose ||dx||^2 is summed over another
    # grid -- x, y, xbar and g of the next iteration are the uninterrupted run's bits, eta agrees to rounding
    begin(f, x0, y0, eta, omega)
    f.objective_iterate(3)
    f.kkt(N.CUR, omega)
    assert torch.equal(gradient(f), three[1])                               # (the pass formed the same g of the same x)
    f.objective_iterate(1)
    begin(e, x0, y0, eta, omega)
    e.objective_iterate(4)
    a, b = full(e), full(f)
    assert all(torch.equal(u, v) for u, v in zip(a[0][0], b[0][0])) and torch.equal(a[1], b[1])      # (x, y, xbar, the sums; g)
    # of the four sums only ||dx||^2 is added up otherwise: the same terms in double in another order, (number of terms) 2^-53 of it
    ra, rb = host(a[2]), host(b[2])
    assert ra[1] == rb[1] and ra[2] == rb[2] and ra[3] == rb[3] and abs(ra[0] - rb[0]) <= qp.n * 2.0 ** -53 * ra[0], (ra, rb)
    sa, sb = a[0][1], b[0][1]
    assert all(sa[k] == sb[k] for k in ("omega", "k", "accepted", "denominator", "curvature")), (sa, sb)
    for k in ("eta", "tau", "sigma", "w_pending", "eta_sum", "eta_bar"):                 # (what follows from ||dx||^2: to rounding)
        close([sb[k]], [sa[k]], dtype, k + " behind a kept K'y")
    # the fixed step on the same handle, before and after adaptive iterations: the bits of a fresh handle
    fresh = lp.engine(dtype, quad_matrix=qp.Q)
    begin(fresh, x0, y0, eta, omega)
    fresh.iterate(3, False)
    want = state(fresh, FIXED_SCALARS), gradient(fresh)
    begin(e, x0, y0, eta, omega)
    e.iterate(3, False)
    got = state(e, FIXED_SCALARS), gradient(e)
    assert same(want[0], got[0]) and torch.equal(want[1], got[1])
    begin(e, x0, y0, eta, omega)
    e.objective_iterate(3)
    begin(e, x0, y0, eta, omega)
    e.iterate(3, False)
    got = state(e, FIXED_SCALARS), gradient(e)
    assert same(want[0], got[0]) and torch.equal(want[1], got[1])
    # ... and in one sequence: adaptive, fixed, adaptive -- each leg from the point and step the other left, as a fresh handle takes it
    begin(e, x0, y0, eta, omega)
    e.objective_iterate(2)
    x, y = e.get_iterate(N.CUR)
    sc = e.scalars()
    e.iterate(2, False)
    begin(fresh, host(x), host(y), sc["eta"], omega)
    fresh.iterate(2, False)
    assert all(torch.equal(u, v) for u, v in zip(e.get_iterate(N.CUR), fresh.get_iterate(N.CUR)))
    assert torch.equal(gradient(e), gradient(fresh))
    x, y = e.get_iterate(N.CUR)
    sc = e.scalars()
    e.objective_iterate(1)                                                  # (the fixed half-steps lowered g_cur: formed anew)
    fresh.set_iterate(x, y)
    fresh.set_step(sc["eta"], omega, 1.0, int(sc["k"]))
    fresh.objective_iterate(1)
    # (K dx comes from a K x carried along on one handle and multiplied anew on the other: dy'K dx agrees to rounding, the rest in bits)
    pick = lambda eng: list(eng.get_iterate(N.CUR)) + [gradient(eng), eng.buffer(N.BUF_RED)[[0, 1, 3]]]
    assert all(torch.equal(u, v) for u, v in zip(pick(e), pick(fresh)))
    se, sf = e.scalars(), fresh.scalars()
    assert all(se[k] == sf[k] for k in ("accepted", "curvature", "k")) and se["curvature"] > 0
    close([se["eta"]], [sf["eta"]], dtype, "eta after fixed iterations")
    # a bare dual half-step moves the iterate too (it swaps the buffers: x goes back to the one before the last step while the buffer
    # holds g of the last): the iteration behind it forms the gradient of the x it starts from, as a fresh handle does
    begin(e, x0, y0, eta, omega)
    e.objective_iterate(2)
    x2 = e.get_iterate(N.CUR)[0]
    N.check(e.lib.pdlp_dual_half(e.h, 0), "pdlp_dual_half")
    x, y = e.get_iterate(N.CUR)
    assert not torch.equal(x, x2)
    sc = e.scalars()
    e.objective_iterate(1)
    fresh.set_iterate(x, y)
    fresh.set_step(sc["eta"], omega, 1.0, int(sc["k"]))
    fresh.objective_iterate(1)
    assert all(torch.equal(u, v) for u, v in zip(pick(e), pick(fresh)))


# ---------------------------------------------------------------------------------------------------
# 4. whole solves: the seed-1 rows of the table in DESIGN.md 4.5.1
# ---------------------------------------------------------------------------------------------------
SOLVES = [row for row in TABLE if row[5] == 1]


def solve(qp, dtype, tol, **kw):
    t = lambda v: dev(v, dtype)
    problem = (t(qp.c), tp.CsrPair.from_any(qp.A, device=DEV, dtype=dtype), t(qp.q), qp.m_ineq, t(qp.l), t(qp.u))
    return tp.solve_lp(problem, tol=tol, dtype=dtype, seed=3, primal_weight_update=True, quad_matrix=qp.Q, **kw)


def check_solution(res, qp, tol, tag, Q=None, d=None):
    print(f"{tag}: k={res.iterations} n={res.restarts} j={res.kkt_passes} objective {res.objective:.10g} (opt {qp.opt:.10g}) "
          f"rel {res.rel_primal_residual:.3g} {res.rel_dual_residual:.3g} {res.rel_gap:.3g}")
    assert res.status == "Solved", (tag, res.status, res.iterations)
    assert abs(res.objective - qp.opt) <= bound_of(tol, qp.opt), (tag, res.objective, qp.opt)
    assert max(res.rel_primal_residual, res.rel_dual_residual, res.rel_gap) <= tol, tag
    x = host(res.x).reshape(-1)
    assert (x >= qp.l).all() and (x <= qp.u).all(), tag
    assert abs(float(qp.c @ x + 0.5 * x @ (qp.Q @ x) + 0.5 * np.sum(qp.d * x * x)) - res.objective) <= 1e-2


@pytest.mark.parametrize("row", SOLVES, ids=lambda r: f"{r[0]}x{r[1]}_{r[3]}_{r[4]:g}")
def test_solve_the_table_in_float64_with_the_models_counts(row):
    m, n, per_row, kind, tol, seed = row
    _, (iters, restarts), _ = TABLE[row]
    qp = qp_of(m, n, per_row, kind, seed)
    res = solve(qp, torch.float64, tol, quad_step="adaptive")
    check_solution(res, qp, tol, f"{m} x {n} {kind} adaptive f64 tol {tol:g}")
    assert (res.iterations, res.restarts) == (iters, restarts)
    # the accounting of an adaptive LP solve: one pass per iteration, three per check, two per restart
    assert res.kkt_passes == iters + 3 * (iters // 40) + 2 * restarts


@pytest.mark.parametrize("row", [r for r in SOLVES if r[4] == 1e-4], ids=lambda r: f"{r[0]}x{r[1]}_{r[3]}")
def test_solve_the_table_in_float32_below_the_fixed_steps_count(row):
    m, n, per_row, kind, tol, seed = row
    qp = qp_of(m, n, per_row, kind, seed)
    fixed = solve(qp, torch.float32, tol)
    res = solve(qp, torch.float32, tol, quad_step="adaptive")
    check_solution(fixed, qp, tol, f"{m} x {n} {kind} fixed f32")
    check_solution(res, qp, tol, f"{m} x {n} {kind} adaptive f32")
    assert res.iterations < fixed.iterations
    again = solve(qp, torch.float32, tol, quad_step="fixed")                # (the default is the fixed step, bit for bit)
    assert (again.iterations, again.restarts, again.kkt_passes, again.objective) == (fixed.iterations, fixed.restarts, fixed.kkt_passes,
                                                                                    fixed.objective)
    assert torch.equal(again.x, fixed.x)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.float64, 1e-8)], ids=DT_IDS)
def test_solve_with_ruiz_and_pock_chambolle(dtype, tol):
    qp = qp_of(37, 23, None, "lowrank")
    res = solve(qp, dtype, tol, quad_step="adaptive", precondition=True, pock_chambolle=True)
    x = host(res.x).reshape(-1)
    eps = 4 * float(np.finfo(NP[dtype]).eps)                                 # (un-scaled x: the rounding of D_col * (l / D_col))
    assert (x >= qp.l - eps * np.abs(np.where(np.isfinite(qp.l), qp.l, 0))).all() and (x <= qp.u + eps * np.abs(np.where(np.isfinite(qp.u), qp.u, 0))).all()
    print(f"37 x 23 Ruiz + Pock-Chambolle adaptive: k={res.iterations} n={res.restarts} objective {res.objective:.10g} (opt {qp.opt:.10g})")
    assert res.status == "Solved"
    assert abs(res.objective - qp.opt) <= bound_of(tol, qp.opt)
    assert max(res.rel_primal_residual, res.rel_dual_residual, res.rel_gap) <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_solve_with_quad_diag_and_q_upper(dtype):
    """the 600 x 520 instance with the diagonal term as well and upper sides on the inequality rows that x* respects (on the active
    rows half a unit above q, on the inactive ones half a unit above K x*): the optimum stays, the prox division stays in the
    half-step and only Q's curvature enters the rule"""
    tol = 1e-4
    qp = qp_of(600, 520, 8, "sparse", diag=True)
    assert (qp.d > 0).sum() > 100
    ineq = np.arange(qp.m) < qp.m_ineq
    qu = np.where(ineq, np.maximum(qp.q, qp.A @ qp.xs) + 0.5, INF)
    res = solve(qp, dtype, tol, quad_step="adaptive", quad_diag=dev(qp.d, dtype), q_upper=dev(qu, dtype))
    check_solution(res, qp, tol, f"600 x 520 with quad_diag and q_upper adaptive {dtype}")
    fixed = solve(qp, dtype, tol, quad_diag=dev(qp.d, dtype), q_upper=dev(qu, dtype))
    assert fixed.status == "Solved"
    print(f"    the fixed step: k={fixed.iterations} n={fixed.restarts}")


# ---------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------
def test_refusals():
    qp = qp_of(37, 23, None, "lowrank")
    lp = lp_of(qp)
    dtype = torch.float32
    lib = N.load()
    x0, y0 = start_point(qp, dtype)

    def refused(eng, what):
        rc = lib.pdlp_objective_iterate(eng.h, 1)
        assert rc != 0 and "call sequence" in lib.pdlp_strerror(rc).decode(), (what, rc)
        with pytest.raises(N.PdlpError, match="call sequence"):
            eng.objective_iterate(1)
    # without Q: a plain handle, one with graph replay, mixed precision with and without delta mode, a shard, a shard with a peer
    # exchange connected
    e = lp.engine(dtype)
    begin(e, x0, y0, 0.05, 0.8)
    refused(e, "no Q")
    e.set_option(N.OPT_GRAPH, 1)
    refused(e, "graph replay")
    e.set_option(N.OPT_GRAPH, 0)
    for delta in (True, False):
        refused(lp.engine(torch.float32, vec_dtype=torch.float64, delta=delta), f"mixed, delta={delta}")
    from tests.host_lp import get_lp
    from tests.shard_world import World
    world = World(get_lp("mid"), 2, torch.float32, None)
    refused(world.engs[0], "a shard")
    peer = world.engs[1]
    assert lib.pdlp_peer_connect(peer.h, 1, 2, None, N.PEER_LOOPBACK) == 0 and peer.peer_status()["connected"]
    refused(peer, "a peer exchange")
    assert lib.pdlp_objective_iterate(None, 1) == lib.pdlp_objective_iterate(e.h, -1) == -1
    # a handle on which the Halpern iteration has run: PDLP_AVG holds its candidate until the next set_iterate
    e.halpern_iterate(2)
    e.set_objective_matrix(qp.Q)
    refused(e, "Halpern")
    begin(e, x0, y0, 0.05, 0.8)
    e.objective_iterate(2)
    e.objective_iterate(0)
    # taken away again
    e.set_objective_matrix(None)
    refused(e, "Q taken away")
    e.iterate(2, True)
    # after the new call every refusal of a handle with Q still holds -- the whole table of tests/test_gpu_quad_matrix.py and the
    # checks beside it -- and the fixed step still runs
    e.set_objective_matrix(qp.Q)
    begin(e, x0, y0, 0.05, 0.8)
    e.objective_iterate(2)
    X, Y = torch.zeros(qp.n, 8, device=DEV), torch.zeros(qp.m, 8, device=DEV)
    st, diag = N.C.c_int32(0), (N.C.c_double * 8)()
    still = {
        "iterate adaptive": lambda: e.iterate(1, True),
        "primal_half adaptive": lambda: N.check(lib.pdlp_primal_half(e.h, 1), "pdlp_primal_half"),
        "dual_half adaptive": lambda: N.check(lib.pdlp_dual_half(e.h, 1), "pdlp_dual_half"),
        "adaptive_retry": e.adaptive_retry,
        "adaptive_reduce": lambda: N.check(lib.pdlp_adaptive_reduce(e.h), "pdlp_adaptive_reduce"),
        "adaptive_update": lambda: N.check(lib.pdlp_adaptive_update(e.h), "pdlp_adaptive_update"),
        "halpern_iterate": lambda: e.halpern_iterate(1),
        "halpern_fixed_point": e.halpern_fixed_point,
        "infeas_reset": e.infeas_reset,
        "detect_infeasibility": lambda: e.detect_infeasibility(1e-4),
        "infeas_local": lambda: N.check(lib.pdlp_infeas_local(e.h, 1e-4), "pdlp_infeas_local"),
        "infeas_finish": lambda: N.check(lib.pdlp_infeas_finish(e.h, 1e-4, N.C.byref(st), diag), "pdlp_infeas_finish"),
        "mv_steps": lambda: e.mv_steps(X, Y, 1, 0.1, 0.8), "mv_gap": lambda: e.mv_gap(X, Y), "mv_product": lambda: e.mv_product(X),
        "set_delta": lambda: e.set_delta(True),
        "graph replay": lambda: e.set_option(N.OPT_GRAPH, 1),
    }
    for name, call in still.items():
        with pytest.raises(N.PdlpError, match="call sequence"):
            call()
        assert name
    ident = (N.C.c_char * 128)()
    assert lib.pdlp_comm_init(e.h, None, ident, 0, 1) == lib.pdlp_infeas_begin(e.h) != 0       # (the same refusal)
    assert lib.pdlp_peer_connect(e.h, 0, 2, None, 0) != 0
    # every batch call, on a handle that has run the new iteration
    from torchpdlp_amd.batch import BatchEngine
    t = lambda v: dev(v, dtype)
    K = tp.CsrPair(lp.m, lp.n, dev(lp.A.indptr, torch.int32), dev(lp.A.indices, torch.int32), t(lp.A.data))
    be = BatchEngine(K, lp.m_ineq, t(lp.c), t(lp.q), t(lp.l), t(lp.u), 2)
    V = torch.ones(lp.n, be.Bp, device=DEV)
    be.eng.set_objective_matrix(qp.Q)
    begin(be.eng, x0, y0, 0.05, 0.8)
    be.eng.objective_iterate(2)
    with pytest.raises(N.PdlpError, match="call sequence"):
        be.product(V)
    with pytest.raises(N.PdlpError, match="call sequence"):
        be.iterate(1, False, 0)
    be.eng.set_objective_matrix(None)
    be.product(V)
    before = [v.clone() for v in e.get_iterate(N.CUR)]
    e.objective_iterate(1)                                                  # (none of the refused calls disturbed the handle)
    e.iterate(1, False)
    assert not torch.equal(before[0], e.get_iterate(N.CUR)[0])
    # the size query counts the partial sums of the curvature: the engine allocates what it reports
    nb, nb_more = N.C.c_int64(0), N.C.c_int64(0)
    N.check(lib.pdlp_objective_matrix_bytes(e.h, 0, N.C.byref(nb)), "bytes")
    N.check(lib.pdlp_objective_matrix_bytes(e.h, 10_000_000, N.C.byref(nb_more)), "bytes")
    assert nb.value % 256 == 0 and nb_more.value > nb.value + (2048 + 64) * 4 * 8 - 256
