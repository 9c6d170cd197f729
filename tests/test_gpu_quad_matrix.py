"""The sparse quadratic objective c'x + 1/2 x'Qx on the GPU (pdlp_set_objective_matrix, PdlpEngine(quad_matrix=),
solve_lp(quad_matrix=)): the plain product with Q exactly, six iterations of the linearised step with the KKT and report numbers
against the float64 numpy model of tests/qp_model.py, a Q without stored entries against an engine that never heard of it bit for
bit, Q together with the diagonal term and two-sided rows, the handle's state around the new calls, and whole solves of problems with
a constructed optimum."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import torchpdlp_amd as tp
from tests.host_lp import DEV, NP, HostLP
from tests.qp_model import KINDS, GeneralQuadModel, make_general_qp, quad_matrix_of
from torchpdlp_amd import _native as N

DTYPES = [torch.float32, torch.float64]
DT_IDS = ["f32", "f64"]
INF = float("inf")
_QPS = {}


@pytest.fixture(scope="module", autouse=True)
def _setup():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    N.load()


def dev(v, dtype):
    return torch.tensor(np.asarray(v), dtype=dtype, device=DEV)


def host(v):
    return v.detach().cpu().numpy().astype(np.float64)


def tols(dtype):
    """what tests/test_gpu_quad.py grants the same quantities"""
    return (1e-4, 2e-5) if dtype == torch.float32 else (1e-10, 1e-10)


def close(got, ref, dtype, tag=""):
    rtol, atol = tols(dtype)
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(ref, np.float64), rtol=rtol, atol=atol, err_msg=tag)


def assert_dict(got, ref, dtype, tag):
    for key in ("pr", "dr", "gap", "p", "d_adj", "kkt"):
        close(got[key], float(ref[key]), dtype, f"{tag}:{key}")


def qp_of(m, n, per_row, kind, diag=False):
    key = (m, n, per_row, kind, diag)
    if key not in _QPS:
        _QPS[key] = make_general_qp(m, n, 1, per_row, kind, diag=diag)
    return _QPS[key]


def scaling_of(qp):
    """factors that make the problem the scaled form of another one: powers of two, so every number stays a float32 number"""
    rng = np.random.default_rng(77)
    return 2.0 ** rng.integers(-1, 2, qp.n), 2.0 ** rng.integers(-1, 2, qp.m)


def lp_of(qp, scaled=False):
    dc, dr = scaling_of(qp) if scaled else (None, None)
    return HostLP(qp.A, qp.m_ineq, qp.c, qp.q, qp.l, qp.u, dc, dr)


def model_of(qp, matrix=True, qu=None):
    return GeneralQuadModel(qp.A, qp.m_ineq, qp.c, qp.q, qp.l, qp.u, qp.Q if matrix else None, qp.d, qu)


def start_point(qp, dtype, seed=3):
    rng = np.random.default_rng(seed)
    lo, hi = np.where(np.isinf(qp.l), -3, qp.l), np.where(np.isinf(qp.u), 3, qp.u)
    x = np.clip(rng.standard_normal(qp.n), lo, hi)
    y = rng.standard_normal(qp.m)
    y[:qp.m_ineq] = np.abs(y[:qp.m_ineq])
    return [v.astype(NP[dtype]).astype(np.float64) for v in (x, y)]


def steps_of(lp, Q, dtype, omega=0.8):
    """a step of the linearised iteration: rules.qp_eta from exact norms, and tau, sigma as k_set_step rounds them"""
    from torchpdlp_amd.rules import qp_eta
    T = NP[dtype]
    L = float(np.linalg.norm(Q.toarray(), 2)) if Q is not None and Q.nnz else 0.0
    eta = float(qp_eta(lp.norm2(), L, omega, T))
    return eta, omega, float(T(eta) / T(omega)), float(T(eta) * T(omega))


def begin(e, x, y, eta, omega):
    e.set_iterate(dev(x, e.dtype), dev(y, e.dtype))
    e.set_step(float(eta), float(omega), 1.0, 0)


def gradient(e):
    """g = c + Q x of the point the engine last looked at"""
    return e.buffer(N.BUF_LAM_PREV).clone()


# ---------------------------------------------------------------------------------------------------
# 1. the plain product, exactly
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [23, 520, 2600])
@pytest.mark.parametrize("kind", KINDS)
def test_objective_product_is_the_dense_product_exactly(kind, n, dtype):
    """every entry of Q and x is a small dyadic rational, so every partial sum is exact in float32 and the order of the additions
    cannot matter: one row block (23), several (520), and the chunks of a row longer than the block (arrow at 2600)"""
    Q = quad_matrix_of(n, 1, kind)
    rng = np.random.default_rng(n)
    lp = HostLP(np.eye(2, n), 1, np.zeros(n), np.zeros(2), -np.ones(n), np.ones(n))
    e = lp.engine(dtype, quad_matrix=Q)
    assert e.quad_matrix is not None and e.quad_matrix.nnz == Q.nnz
    if kind == "arrow" and n > 2048:
        assert int(np.diff(Q.indptr).max()) > 2048                          # (the long-row chunks run)
    for _ in range(2):
        x = rng.integers(-4, 5, n) / 4.0
        want = Q.toarray() @ x
        assert np.array_equal(want.astype(NP[dtype]).astype(np.float64), want)
        got = e.objective_product(dev(x, dtype))
        assert torch.equal(got, dev(want, dtype))
    assert np.abs(want).max() > 0.5


# ---------------------------------------------------------------------------------------------------
# 2. six iterations, the KKT numbers and the report against the model
# ---------------------------------------------------------------------------------------------------
# (the dense rows of the 37 x 23 K do not fit the tile format -- build_tiles declines them -- so its second form is the sorted copy)
CASES = {"37x23-csr": (37, 23, None, "lowrank", "csr"), "37x23-sorted": (37, 23, None, "lowrank", "sorted"),
         "600x520-csr": (600, 520, 8, "sparse", "csr"), "600x520-tiles": (600, 520, 8, "sparse", "tiles")}


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", list(CASES))
def test_six_iterations_kkt_and_report_against_the_model(case, dtype):
    m, n, per_row, kind, form = CASES[case]
    qp = qp_of(m, n, per_row, kind)
    lp = lp_of(qp, scaled=True)
    mo, lin = model_of(qp), model_of(qp, matrix=False)
    eta, omega, tau, sigma = steps_of(lp, qp.Q, dtype)
    x0, y0 = start_point(qp, dtype)
    e = lp.engine(dtype, form, quad_matrix=qp.Q)
    assert e.quad_matrix is not None
    if form == "tiles":
        assert all(k.startswith("tiled") for k in e.kernels), e.kernels
    begin(e, x0, y0, eta, omega)
    e.iterate(6, False)
    mx, my, xs, ys = x0, y0, [], []
    for _ in range(6):
        px, py = mx, my
        mx, my, mxbar, _ = mo.step(mx, my, tau, sigma)
        xs.append(mx)
        ys.append(my)
    lx, ly = x0, y0
    for _ in range(6):
        lx, ly, _, _ = lin.step(lx, ly, tau, sigma)
    xg, yg = e.get_iterate(N.CUR)
    close(host(xg), mx, dtype, "x")
    close(host(yg), my, dtype, "y")
    close(host(e.buffer(N.BUF_XBAR)), mxbar, dtype, "xbar")
    close(host(gradient(e)), mo.grad(px), dtype, "g")                       # (of the x the last primal half-step started from)
    rtol, atol = tols(dtype)
    assert np.max(np.abs(mx - lx)) > 100 * (atol + rtol * np.max(np.abs(mx)))       # (an implementation that ignores Q is far off)
    xp, yp = e.get_iterate(N.PREV)
    close(host(xp), px, dtype, "x_prev")
    close(host(yp), py, dtype, "y_prev")
    # the KKT pass at the current iterate first (it keeps K'y, which closes the running sums), then the average from the sums
    got = {N.CUR: e.kkt(N.CUR, omega)}
    close(host(gradient(e)), mo.grad(mx), dtype, "g of the KKT pass")
    e.flush_average(False)
    e.compute_average()
    xa, ya = e.get_iterate(N.AVG)
    close(host(xa), np.mean(xs, axis=0), dtype, "x_avg")
    close(host(ya), np.mean(ys, axis=0), dtype, "y_avg")
    got[N.AVG] = e.kkt(N.AVG, omega)
    got[N.PREV] = e.kkt(N.PREV, omega)
    for which in (N.CUR, N.AVG, N.PREV):
        x, y = (host(v) for v in e.get_iterate(which))
        ref = mo.kkt(x, y, omega)
        assert_dict(got[which], ref, dtype, f"{case}:kkt({which})")
        hq = 0.5 * float(x @ (mo.Q @ x))
        assert hq > 1e-2 * (1 + abs(ref["p"]))                              # (the term is a visible part of both objectives)
        for unscaled in (False, True):
            dd = (lp.d_col, lp.d_row) if unscaled else (None, None)
            ref = mo.kkt(x, y, omega, *dd)
            sums, lam = mo.sums(x, y, *dd)
            tag = f"{case}:which={which}:unscaled={unscaled}"
            assert_dict(e.kkt(which, omega, unscaled=unscaled), ref, dtype, "kkt " + tag)
            # the slot convention: PDLP_BUF_RED[3] = c'x + h, [1] = l'lam+ - h
            red = host(e.buffer(N.BUF_RED))
            for slot in (1, 3):
                np.testing.assert_allclose(red[slot], sums[slot], rtol=rtol, atol=atol * max(1.0, abs(sums[3])), err_msg=f"slot {slot} " + tag)
            close(red[N.NRED - 1], 2 * hq, dtype, "x'Qx " + tag)
            rep = e.report(which, unscaled=unscaled, omega=omega)
            assert_dict(rep, ref, dtype, "report " + tag)
            close(host(rep["reduced_costs"]), lam, dtype, "reduced costs " + tag)
            close(host(rep["row_activity"]), (lp.A @ x) / (lp.d_row if unscaled else 1.0), dtype, "row activity " + tag)
    # the passes changed nothing of the iteration: six more steps continue the model's
    e.iterate(1, False)
    nx, ny, _, _ = mo.step(mx, my, tau, sigma)
    close(host(e.get_iterate(N.CUR)[0]), nx, dtype, "x after the passes")
    close(host(e.get_iterate(N.CUR)[1]), ny, dtype, "y after the passes")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form", ["csr", "tiles"])
def test_kkt_at_the_average_from_the_running_sums_still_sees_q_x_avg(form, dtype):
    """kkt(AVG) after kkt(CUR), flush_average and compute_average takes K'y_avg and K x_avg from the running sums -- with the y of the
    averaged iterate overwritten in between, the dual residual is still the one of the TRUE average -- but multiplies Q x_avg: the
    residual is the quadratic problem's, and x_avg overwritten instead moves it"""
    qp = qp_of(600, 520, 8, "sparse")
    lp = lp_of(qp)
    mo, lin = model_of(qp), model_of(qp, matrix=False)
    eta, omega, _, _ = steps_of(lp, qp.Q, dtype)
    x0, y0 = start_point(qp, dtype)
    e = lp.engine(dtype, form, quad_matrix=qp.Q)

    def averaged():
        begin(e, x0, y0, eta, omega)
        e.iterate(40, False)
        e.kkt(N.CUR, omega)
        e.flush_average(False)
        e.compute_average()
        return [host(v) for v in e.get_iterate(N.AVG)]
    xa, ya = averaged()
    e.buffer(N.BUF_Y_AVG)[:] += 1.0
    got = e.kkt(N.AVG, omega)
    true, moved, without = mo.kkt(xa, ya, omega), mo.kkt(xa, ya + 1.0, omega), lin.kkt(xa, ya, omega)
    assert abs(true["dr"] - moved["dr"]) > 1.0 and abs(true["dr"] - without["dr"]) > 1.0
    close(got["dr"], true["dr"], dtype, "dr")
    close(got["pr"], true["pr"], dtype, "pr")
    # the product with Q is multiplied out: it follows the buffer of x_avg, while K x_avg (from the sums) does not
    xa, ya = averaged()
    e.buffer(N.BUF_X_AVG)[:] += 0.5
    got = e.kkt(N.AVG, omega)
    ref = GeneralQuadModel(qp.A, qp.m_ineq, qp.c + mo.Q @ np.full(qp.n, 0.5), qp.q, qp.l, qp.u, qp.Q).kkt(xa, ya, omega)
    close(got["dr"], ref["dr"], dtype, "dr with x_avg overwritten")
    close(got["pr"], mo.kkt(xa, ya, omega)["pr"], dtype, "pr with x_avg overwritten")


# ---------------------------------------------------------------------------------------------------
# 3. a Q without stored entries: the bits of an engine on which the setter was never called
# ---------------------------------------------------------------------------------------------------
def everything(e, qp, x0, y0, eta, omega):
    out, dicts = [], []
    begin(e, x0, y0, eta, omega)
    e.iterate(6, False)
    out += list(e.get_iterate(N.CUR)) + [e.buffer(N.BUF_XBAR).clone()]
    dicts.append(e.kkt(N.CUR, omega))
    out.append(e.buffer(N.BUF_RED)[:6].clone())
    e.flush_average(False)
    e.compute_average()
    out += list(e.get_iterate(N.AVG))
    for which in (N.AVG, N.PREV, N.CUR):
        for unscaled in (False, True):
            dicts.append(e.kkt(which, omega, unscaled=unscaled))
            out.append(e.buffer(N.BUF_RED)[:6].clone())
            rep = e.report(which, unscaled=unscaled, omega=omega)
            out += [rep.pop("y"), rep.pop("reduced_costs"), rep.pop("row_activity")]
            dicts.append(rep)
    e.restart(N.AVG)
    e.iterate(3, False)
    out += list(e.get_iterate(N.CUR))
    sc = e.scalars()
    dicts.append({k: sc[k] for k in ("eta", "omega", "tau", "sigma", "eta_sum", "k", "w_pending")})
    return out, dicts


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form", ["csr", "tiles"])
def test_a_matrix_without_entries_changes_no_bit(form, dtype):
    import scipy.sparse as sp
    qp = qp_of(600, 520, 8, "sparse")
    lp = lp_of(qp, scaled=True)
    eta, omega, _, _ = steps_of(lp, None, dtype)
    x0, y0 = start_point(qp, dtype)
    plain = lp.engine(dtype, form)
    zero = lp.engine(dtype, form, quad_matrix=sp.csr_matrix((qp.n, qp.n)))
    assert plain.quad_matrix is None and zero.quad_matrix is not None and zero.quad_matrix.nnz == 0
    (va, da), (vb, db) = everything(plain, qp, x0, y0, eta, omega), everything(zero, qp, x0, y0, eta, omega)
    assert len(va) == len(vb) and all(torch.equal(a, b) for a, b in zip(va, vb))
    assert da == db
    assert torch.equal(zero.objective_product(dev(x0, dtype)), torch.zeros(qp.n, dtype=dtype, device=DEV))


def test_detaching_restores_the_results_of_the_lp():
    dtype = torch.float32
    qp = qp_of(600, 520, 8, "sparse")
    lp = lp_of(qp)
    eta, omega, _, _ = steps_of(lp, qp.Q, dtype)
    x0, y0 = start_point(qp, dtype)
    plain, e = lp.engine(dtype), lp.engine(dtype, quad_matrix=qp.Q)
    begin(e, x0, y0, eta, omega)
    e.iterate(5, False)
    with_q = e.get_iterate(N.CUR)[0].clone()
    e.kkt(N.CUR, omega)
    e.flush_average(False)
    e.compute_average()
    e.kkt(N.AVG, omega)
    e.restart(N.AVG)
    e.set_objective_matrix(None)
    assert e.quad_matrix is None
    with pytest.raises(N.PdlpError, match="call sequence"):
        e.objective_product(dev(x0, dtype))
    outs = []
    for eng in (plain, e):
        begin(eng, x0, y0, eta, omega)
        eng.iterate(6, False)
        kk = eng.kkt(N.CUR, omega)
        outs.append((list(eng.get_iterate(N.CUR)) + [eng.buffer(N.BUF_XBAR).clone()], kk))
    assert all(torch.equal(a, b) for a, b in zip(outs[0][0], outs[1][0])) and outs[0][1] == outs[1][1]
    begin(plain, x0, y0, eta, omega)
    plain.iterate(5, False)
    assert not torch.equal(with_q, plain.get_iterate(N.CUR)[0])             # (Q was at work in between)
    # ... and the adaptive step, refused while Q was set, runs again
    e.iterate(2, True)


# ---------------------------------------------------------------------------------------------------
# 4. together with the diagonal term and two-sided rows
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form", ["csr", "tiles"])
def test_q_with_quad_diag_and_q_upper(form, dtype):
    qp = qp_of(600, 520, 8, "sparse", diag=True)
    assert (qp.d > 0).sum() > 100
    lp = lp_of(qp)
    i = np.arange(qp.m)
    ineq = i < qp.m_ineq
    qu = np.full(qp.m, INF)
    qu[ineq & (i % 4 == 1)] = qp.q[ineq & (i % 4 == 1)]
    qu[ineq & (i % 4 >= 2)] = qp.q[ineq & (i % 4 >= 2)] + 0.5
    mo = model_of(qp, qu=qu)
    eta, omega, tau, sigma = steps_of(lp, qp.Q, dtype)
    rng = np.random.default_rng(19)
    x0, _ = start_point(qp, dtype)
    y0 = rng.standard_normal(qp.m).astype(NP[dtype]).astype(np.float64)     # (either sign)
    e = lp.engine(dtype, form, quad_matrix=qp.Q, quad_diag=dev(qp.d, dtype), q_upper=dev(qu, dtype))
    assert e.quad_matrix is not None and e.quad_diag is not None and e.q_upper is not None
    begin(e, x0, y0, eta, omega)
    e.iterate(6, False)
    mx, my = x0, y0
    for _ in range(6):
        mx, my, _, _ = mo.step(mx, my, tau, sigma)
    assert (my[:qp.m_ineq] < -0.01).sum() > 10                               # (upper sides are active)
    xg, yg = e.get_iterate(N.CUR)
    close(host(xg), mx, dtype, "x")
    close(host(yg), my, dtype, "y")
    x, y = host(xg), host(yg)
    ref = mo.kkt(x, y, omega)
    assert_dict(e.kkt(N.CUR, omega), ref, dtype, "kkt")
    rep = e.report(N.CUR, omega=omega)
    assert_dict(rep, ref, dtype, "report")
    close(host(rep["reduced_costs"]), mo.sums(x, y)[1], dtype, "reduced costs")
    # each of the three matters at this point
    for other in (GeneralQuadModel(qp.A, qp.m_ineq, qp.c, qp.q, qp.l, qp.u, None, qp.d, qu), GeneralQuadModel(qp.A, qp.m_ineq, qp.c, qp.q, qp.l, qp.u, qp.Q, None, qu),
                  model_of(qp)):
        o = other.kkt(x, y, omega)
        assert max(abs(o[k] - ref[k]) for k in ("pr", "dr", "p")) > 1e-2


# ---------------------------------------------------------------------------------------------------
# 5. state
# ---------------------------------------------------------------------------------------------------
def test_calls_and_handles_without_the_matrix_are_refused():
    qp = qp_of(37, 23, None, "lowrank")
    lp = lp_of(qp)
    dtype = torch.float32
    Qd = tp.CsrPair.from_any(qp.Q, device=DEV, dtype=torch.float64)
    lib = N.load()

    def raw_set(eng, Qp, work=None):
        nb = N.C.c_int64(0)
        N.check(lib.pdlp_objective_matrix_bytes(eng.h, Qp.nnz, N.C.byref(nb)), "bytes")
        work = torch.empty(nb.value + 256, dtype=torch.uint8, device=DEV) if work is None else work
        off = (-work.data_ptr()) % 256
        return lib.pdlp_set_objective_matrix(eng.h, Qp.rowptr.data_ptr(), Qp.colidx.data_ptr(), Qp.val.data_ptr(), work.data_ptr() + off, nb.value), work
    # a mixed-precision handle, in delta mode or not, and a shard of a problem: "call sequence"
    for delta in (True, False):
        em = lp.engine(torch.float32, vec_dtype=torch.float64, delta=delta)
        rc = raw_set(em, Qd)[0]
        assert rc != 0 and "call sequence" in lib.pdlp_strerror(rc).decode()
        with pytest.raises(N.PdlpError, match="call sequence"):
            em.set_objective_matrix(qp.Q)
        assert em.quad_matrix is None
        N.check(lib.pdlp_set_objective_matrix(em.h, None, None, None, None, 0), "detach")       # (taking away what is not there: fine)
    from tests.host_lp import get_lp
    from tests.shard_world import World
    w = World(get_lp("mid"), 2, torch.float32, None)
    sh = w.engs[0]
    import scipy.sparse as sp
    with pytest.raises(N.PdlpError, match="call sequence"):
        sh.set_objective_matrix(sp.identity(sh.n, format="csr"))
    # the workspace: too small, misaligned, missing; one array missing
    e = lp.engine(dtype)
    Qf = tp.CsrPair.from_any(qp.Q, device=DEV, dtype=dtype)
    nb = N.C.c_int64(0)
    N.check(lib.pdlp_objective_matrix_bytes(e.h, Qf.nnz, N.C.byref(nb)), "bytes")
    work = torch.empty(nb.value + 512, dtype=torch.uint8, device=DEV)
    base = work.data_ptr() + (-work.data_ptr()) % 256
    args = (Qf.rowptr.data_ptr(), Qf.colidx.data_ptr(), Qf.val.data_ptr())
    for bad in ((base, nb.value - 1), (base + 8, nb.value), (None, nb.value)):
        rc = lib.pdlp_set_objective_matrix(e.h, *args, *bad)
        assert rc != 0 and "workspace" in lib.pdlp_strerror(rc).decode()
    assert lib.pdlp_set_objective_matrix(e.h, args[0], None, args[2], base, nb.value) == -1
    with pytest.raises(N.PdlpError, match="call sequence"):
        e.objective_product(dev(np.zeros(qp.n), dtype))                    # (no Q yet)
    # graph replay and Q exclude each other, whichever comes first
    e.set_option(N.OPT_GRAPH, 1)
    with pytest.raises(N.PdlpError, match="call sequence"):
        e.set_objective_matrix(qp.Q)
    e.set_option(N.OPT_GRAPH, 0)
    e.set_objective_matrix(qp.Q)
    with pytest.raises(N.PdlpError, match="call sequence"):
        e.set_option(N.OPT_GRAPH, 1)
    e.set_option(N.OPT_GRAPH, 0)
    # while it is set
    x0, y0 = start_point(qp, dtype)
    begin(e, x0, y0, 0.05, 0.8)
    e.iterate(2, False)
    X, Y = torch.zeros(qp.n, 8, device=DEV), torch.zeros(qp.m, 8, device=DEV)
    st, diag = N.C.c_int32(0), (N.C.c_double * 8)()
    refused = {
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
    }
    for name, call in refused.items():
        with pytest.raises(N.PdlpError, match="call sequence"):
            call()
        assert name
    ident = (N.C.c_char * 128)()
    assert lib.pdlp_comm_init(e.h, None, ident, 0, 1) == lib.pdlp_infeas_begin(e.h) != 0       # (the same refusal)
    assert lib.pdlp_peer_connect(e.h, 0, 2, None, 0) != 0
    e.iterate(2, False)                                                     # (none of the refused calls disturbed the handle)
    for bad in (np.ones((qp.n, qp.n + 1)), np.triu(np.ones((qp.n, qp.n))), -np.eye(qp.n)):
        with pytest.raises(ValueError, match="quad_matrix"):
            e.set_objective_matrix(torch.tensor(bad))
    # every batch call
    from torchpdlp_amd.batch import BatchEngine
    t = lambda v: dev(v, dtype)
    K = tp.CsrPair(lp.m, lp.n, dev(lp.A.indptr, torch.int32), dev(lp.A.indices, torch.int32), t(lp.A.data))
    be = BatchEngine(K, lp.m_ineq, t(lp.c), t(lp.q), t(lp.l), t(lp.u), 2)
    V = torch.ones(lp.n, be.Bp, device=DEV)
    be.product(V)
    be.eng.set_objective_matrix(qp.Q)
    with pytest.raises(N.PdlpError, match="call sequence"):
        be.product(V)
    with pytest.raises(N.PdlpError, match="call sequence"):
        be.iterate(1, False, 0)
    be.eng.set_objective_matrix(None)
    be.product(V)
    # taken away: the refused calls run again
    e.set_objective_matrix(None)
    e.infeas_reset()
    e.detect_infeasibility(1e-4)
    e.mv_product(X)
    e.halpern_iterate(1)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_setting_q_drops_a_kept_kty(dtype):
    """a KKT pass at the current iterate keeps K'y and its sums' candidate; pdlp_set_objective_matrix drops both, and the pass after
    it and the half-step after that are the quadratic problem's"""
    qp = qp_of(600, 520, 8, "sparse")
    lp = lp_of(qp)
    mo, lin = model_of(qp), model_of(qp, matrix=False)
    eta, omega, tau, sigma = steps_of(lp, qp.Q, dtype)
    x0, y0 = start_point(qp, dtype)
    e = lp.engine(dtype)
    begin(e, x0, y0, eta, omega)
    e.iterate(3, False)
    x, y = (host(v) for v in e.get_iterate(N.CUR))
    assert_dict(e.kkt(N.CUR, omega), lin.kkt(x, y, omega), dtype, "before")
    e.set_objective_matrix(qp.Q)
    ref = mo.kkt(x, y, omega)
    assert abs(ref["dr"] - lin.kkt(x, y, omega)["dr"]) > 1.0
    assert_dict(e.kkt(N.CUR, omega), ref, dtype, "after")
    e.iterate(1, False)
    nx, ny, _, _ = mo.step(x, y, tau, sigma)
    close(host(e.get_iterate(N.CUR)[0]), nx, dtype, "x")
    close(host(e.get_iterate(N.CUR)[1]), ny, dtype, "y")
    # ... and replacing Q by another one does the same
    Q2 = quad_matrix_of(qp.n, 2, "lowrank")
    e.kkt(N.CUR, omega)
    e.set_objective_matrix(Q2)
    m2 = GeneralQuadModel(qp.A, qp.m_ineq, qp.c, qp.q, qp.l, qp.u, Q2)
    x, y = (host(v) for v in e.get_iterate(N.CUR))
    assert_dict(e.kkt(N.CUR, omega), m2.kkt(x, y, omega), dtype, "replaced")
    e.iterate(1, False)
    close(host(e.get_iterate(N.CUR)[0]), m2.step(x, y, tau, sigma)[0], dtype, "x after the replacement")


# ---------------------------------------------------------------------------------------------------
# 6. whole solves of problems with a constructed optimum (the instances of tests/test_quad_matrix_host.py)
# ---------------------------------------------------------------------------------------------------
SOLVES = {"fixed": {}, "ruiz_pc": dict(precondition=True, pock_chambolle=True)}


def solve_and_check(qp, dtype, tol, mode):
    """the checks of tests/test_gpu_quad.py:solve_and_check"""
    t = lambda v: dev(v, dtype)
    problem = (t(qp.c), tp.CsrPair.from_any(qp.A, device=DEV, dtype=dtype), t(qp.q), qp.m_ineq, t(qp.l), t(qp.u))
    res = tp.solve_lp(problem, tol=tol, dtype=dtype, seed=3, primal_weight_update=True, quad_matrix=qp.Q, **SOLVES[mode])
    print(f"{qp.m} x {qp.n} {mode} tol {tol:g}: k={res.iterations} n={res.restarts} j={res.kkt_passes} objective {res.objective:.10g} "
          f"(opt {qp.opt:.10g}) dual {res.dual_objective:.10g} rel {res.rel_primal_residual:.3g} {res.rel_dual_residual:.3g} {res.rel_gap:.3g}")
    assert res.status == "Solved", (res.status, res.iterations)
    bound = 1e-3 * (1 + abs(qp.opt)) if tol == 1e-4 else 2e-8 * (1 + 2 * abs(qp.opt))
    assert abs(res.objective - qp.opt) <= bound, (res.objective, qp.opt)
    assert max(res.rel_primal_residual, res.rel_dual_residual, res.rel_gap) <= tol, \
        (res.rel_primal_residual, res.rel_dual_residual, res.rel_gap)
    x = host(res.x).reshape(-1)
    eps = 4 * float(np.finfo(NP[dtype]).eps) if "precondition" in SOLVES[mode] else 0.0       # (un-scaled x: the rounding of D_col * (l / D_col))
    lo, hi = qp.l.copy(), qp.u.copy()
    lo[np.isfinite(lo)] -= eps * np.abs(lo[np.isfinite(lo)])
    hi[np.isfinite(hi)] += eps * np.abs(hi[np.isfinite(hi)])
    assert (x >= lo).all() and (x <= hi).all()
    assert abs(float(qp.c @ x + 0.5 * x @ (qp.Q @ x)) - res.objective) <= 1e-2
    assert abs(float(qp.c @ x) - qp.opt) > 10 * bound                                      # (and c'x alone is another number)
    return res


# Mode "ruiz_pc" is the case that needs solve_lp's projection of the returned x onto [l, u]: the last restart adopts the averaged
# iterate, and x_sum / eta_sum of iterates that all sit on the scaled bound l / D_col (not a dyadic number any more) is that bound only
# up to the rounding of the two running sums -- 9 eps outside in float32 and 8 eps in float64 without the projection.
@pytest.mark.parametrize("mode", list(SOLVES))
def test_solve_qp_37x23(mode):
    solve_and_check(qp_of(37, 23, None, "lowrank"), torch.float32, 1e-4, mode)


@pytest.mark.parametrize("mode", list(SOLVES))
def test_solve_qp_37x23_float64(mode):
    solve_and_check(qp_of(37, 23, None, "lowrank"), torch.float64, 1e-8, mode)


def test_solve_qp_tiled_600x520(monkeypatch):
    """PDLP_TILED=1 with 64-column panels puts both products with K of the solve's engine on k_tiled_fused"""
    monkeypatch.setenv("PDLP_TILED", "1")
    monkeypatch.setenv("PDLP_TILE_LW", "6")
    qp = qp_of(600, 520, 8, "sparse")
    t = lambda v: dev(v, torch.float32)
    eng = tp.PdlpEngine.from_full(tp.CsrPair.from_any(qp.A, device=DEV, dtype=torch.float32), t(qp.c), t(qp.q), t(qp.l), t(qp.u), qp.m_ineq,
                                  quad_matrix=qp.Q)
    assert all(k.startswith("tiled") for k in eng.kernels), eng.kernels
    del eng
    solve_and_check(qp, torch.float32, 1e-4, "fixed")


def test_solve_qp_arrow_2600():
    """row and column 0 of Q hold 2600 entries: every product with Q of the solve runs the long-row chunks"""
    solve_and_check(qp_of(300, 2600, 6, "arrow"), torch.float32, 1e-4, "fixed")
