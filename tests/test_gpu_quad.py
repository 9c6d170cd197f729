"""The diagonal quadratic objective c'x + 1/2 x'Dx on the GPU (pdlp_set_objective_diag, PdlpEngine(quad_diag=), solve_lp(quad_diag=)):
six iterations (fixed, adaptive, Halpern) against the float64 numpy model of tests/quad_model.py through every product form, the
KKT and report numbers against the model, all-zero d against an engine that never heard of the term bit for bit, the term together
with two-sided rows, the handle's state around the new call, and whole solves of problems with a constructed optimum."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import torchpdlp_amd as tp
from tests.host_lp import DEV, NP, get_lp
from tests.quad_model import QuadModel, make_qp
from torchpdlp_amd import _native as N

DTYPES = [torch.float32, torch.float64]
INF = float("inf")
EDGE = ["edge_no_ineq", "edge_all_ineq", "edge_empty_row_and_col", "edge_one_by_one", "edge_free_and_fixed"]
# (LP, product form), the list of tests/test_gpu_halpern.py: 37 x 23 and 1 x 1 have one panel; 600 x 520 has several row blocks of K and
# of K' in every form and 9 panels of 64 columns; the dense row and column of `mid_dense` put more items of one row into one tile than it
# holds (the remainder), and those of `long` are longer than the CSR kernel's block: k_long_rows runs the epilogue
SCENARIOS = ([(lp, f) for lp in EDGE for f in ("csr", "sorted", "tiles")] +
             [("mid", f) for f in ("csr", "sorted", "tiles", "tiles_groups")] + [("mid_dense", "tiles_remainder")] +
             [("long", f) for f in ("csr", "sorted", "tiles_remainder")])
IDS = [f"{a}-{b}" for a, b in SCENARIOS]


@pytest.fixture(scope="module", autouse=True)
def _setup():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    N.load()


def dev(v, dtype):
    return torch.tensor(np.asarray(v), dtype=dtype, device=DEV)


def host(v):
    return v.detach().cpu().numpy().astype(np.float64)


def close(got, ref, tol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * max(1.0, float(np.max(np.abs(ref))) if ref.size else 1.0))


def diag_of(lp, seed=31):
    """d for an LP of tests/host_lp.py: multiples of 1/4 in [1/4, 2] with about 40 % zeros (float32 numbers)"""
    rng = np.random.default_rng(seed + lp.n)
    return rng.integers(1, 9, lp.n) / 4.0 * (rng.random(lp.n) >= 0.4)


def model_of(lp, d, qu=None):
    return QuadModel(lp.A, lp.m_ineq, lp.c, lp.q, lp.l, lp.u, d, qu)


def start_points(lp, dtype, seed=3):
    """an anchor and a DIFFERENT iterate, both random (the iterate need not respect the bounds: a Halpern iterate does not)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.where(np.isinf(lp.l), -3, lp.l), np.where(np.isinf(lp.u), 3, lp.u)
    x0 = np.clip(rng.standard_normal(lp.n), lo, hi)
    y0 = rng.standard_normal(lp.m)
    y0[:lp.m_ineq] = np.abs(y0[:lp.m_ineq])
    x1, y1 = x0 + 0.3 * rng.standard_normal(lp.n), y0 + 0.3 * rng.standard_normal(lp.m)
    return [v.astype(NP[dtype]).astype(np.float64) for v in (x0, y0, x1, y1)]


def put(eng, x0, y0, x1, y1, eta, omega):
    """anchor (x0, y0), iterate (x1, y1), t = 0: set_iterate at the anchor, then the iterate written through the buffer views"""
    t = lambda v: torch.tensor(v, dtype=eng.dtype, device=DEV)
    eng.set_iterate(t(x0), t(y0))
    eng.set_step(float(eta), float(omega), 1.0, 0)
    eng.buffer(N.BUF_X_CUR)[:] = t(x1)
    eng.buffer(N.BUF_Y_CUR)[:] = t(y1)


def begin(e, x, y, eta, omega):
    e.set_iterate(dev(x, e.dtype), dev(y, e.dtype))
    e.set_step(float(eta), float(omega), 1.0, 0)


def steps_of(lp, dtype):
    eta, omega = 0.9 / lp.norm2(), 0.8
    T = NP[dtype]
    return eta, omega, float(T(eta) / T(omega)), float(T(eta) * T(omega))          # (tau, sigma as k_set_step rounds them)


# ---------------------------------------------------------------------------------------------------
# 1. six iterations of each mode against the numpy model, in every product form
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name,form", SCENARIOS, ids=IDS)
def test_six_iterations_against_the_model(name, form, dtype):
    lp = get_lp(name)
    eta, omega, tau, sigma = steps_of(lp, dtype)
    d = diag_of(lp)
    mo, lin = model_of(lp, d), model_of(lp, None)
    x0, y0, x1, y1 = start_points(lp, dtype)
    e, p = (lp.engine(dtype, form, quad_diag=dev(d, dtype)) for _ in range(2))
    assert e.quad_diag is not None
    # the tolerance test_gpu_halpern.py grants its six-iteration model comparison in the same precision
    tol = 3e-5 if dtype == torch.float32 else 1e-11
    # fixed step
    begin(e, x1, y1, eta, omega)
    e.iterate(6, False)
    mx, my, lx = x1, y1, x1
    for _ in range(6):
        mx, my, _, _ = mo.step(mx, my, tau, sigma)
    ly = y1
    for _ in range(6):
        lx, ly, _, _ = lin.step(lx, ly, tau, sigma)
    xg, yg = e.get_iterate(N.CUR)
    close(host(xg), mx, tol)
    close(host(yg), my, tol)
    if lp.n >= 20 and (np.isinf(lp.l) | np.isinf(lp.u) | (lp.l < lp.u)).any():
        # an implementation that ignores d would be far off (the LP's own six steps are another point)
        assert np.max(np.abs(mx - lx)) > 100 * tol * max(1.0, np.max(np.abs(mx)))
    # adaptive step (one trial per iteration, kept when rejected; k counts from 1), and the step size it leaves behind
    begin(e, x1, y1, eta, omega)
    e.iterate(6, True)
    mx, my, me = x1, y1, float(eta)
    for it in range(1, 7):
        mx, my, me = mo.adaptive_step(mx, my, me, float(omega), it)
    xg, yg = e.get_iterate(N.CUR)
    close(host(xg), mx, tol)
    close(host(yg), my, tol)
    close([e.scalars()["eta"]], [me], tol)
    # Halpern: anchor (x0, y0), iterate (x1, y1); the candidate is one fixed step of the QUAD PDHG kernels from z, bit for bit
    put(e, x0, y0, x1, y1, eta, omega)
    mx, my = x1, y1
    for it in range(6):
        zx, zy = e.get_iterate(N.CUR)
        e.halpern_iterate(1)
        xc, yc = e.get_iterate(N.AVG)
        p.set_iterate(zx, zy)
        p.set_step(float(eta), float(omega), 1.0, 0)
        p.iterate(1, False)
        px, py = p.get_iterate(N.CUR)
        assert torch.equal(px, xc) and torch.equal(py, yc), it
        assert torch.equal(p.buffer(N.BUF_XBAR), e.buffer(N.BUF_XBAR)), it
        mx, my, mxc, myc = mo.halpern_step(mx, my, x0, y0, it, tau, sigma)
    xg, yg = e.get_iterate(N.CUR)
    for got, ref in ((xg, mx), (yg, my), (xc, mxc), (yc, myc)):
        close(host(got), ref, tol)


# ---------------------------------------------------------------------------------------------------
# 2. the KKT numbers and the report against the model
# ---------------------------------------------------------------------------------------------------
KKT_CASES = [("mid_scaled", f) for f in ("csr", "sorted", "tiles", "tiles_groups")] + [("mid_dense", "tiles_remainder"), ("long", "csr"),
                                                                                      ("edge_free_and_fixed", "csr")]


def assert_dict(got, ref, dtype, tag):
    # float32: what the existing state check grants the same six numbers (tests/test_gpu_halpern.py, check 4)
    rtol, atol = (1e-4, 2e-5) if dtype == torch.float32 else (1e-10, 1e-10)
    for key in ("pr", "dr", "gap", "p", "d_adj", "kkt"):
        np.testing.assert_allclose(got[key], float(ref[key]), rtol=rtol, atol=atol, err_msg=f"{tag}:{key}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name,form", KKT_CASES, ids=[f"{a}-{b}" for a, b in KKT_CASES])
def test_kkt_and_report_against_the_model(name, form, dtype):
    lp = get_lp(name)
    eta, omega, _, _ = steps_of(lp, dtype)
    d = diag_of(lp)
    mo = model_of(lp, d)
    scaled = lp.d_col is not None
    _, _, x1, y1 = start_points(lp, dtype)
    e = lp.engine(dtype, form, quad_diag=dev(d, dtype))
    rtol, atol = (1e-4, 2e-5) if dtype == torch.float32 else (1e-10, 1e-10)
    begin(e, x1, y1, eta, omega)
    e.iterate(40, False)
    got_cur = e.kkt(N.CUR, omega)              # (first: its pass keeps K'y, which closes the running sum)
    e.flush_average(False)
    e.compute_average()
    got_avg = e.kkt(N.AVG, omega)              # the product-free pass over K'y_avg and K x_avg from the running sums
    for which, got in ((N.CUR, got_cur), (N.AVG, got_avg)):
        x, y = (host(v) for v in e.get_iterate(which))
        ref = mo.kkt(x, y, omega)
        assert_dict(got, ref, dtype, f"{name}:{form}:kkt({which})")
        assert mo.half(x) > 1e-2 * (1 + abs(ref["p"]))                       # (the term is a visible part of both objectives)
        for unscaled in ((False, True) if scaled else (False,)):
            dd = (lp.d_col, lp.d_row) if unscaled else (None, None)
            ref = mo.kkt(x, y, omega, *dd)
            _, lam = mo.sums(x, y, *dd)
            tag = f"{name}:{form}:which={which}:unscaled={unscaled}"
            assert_dict(e.kkt(which, omega, unscaled=unscaled), ref, dtype, "kkt " + tag)
            rep = e.report(which, unscaled=unscaled, omega=omega)
            assert_dict(rep, ref, dtype, "report " + tag)
            np.testing.assert_allclose(host(rep["reduced_costs"]), lam, rtol=rtol, atol=atol, err_msg=tag)
            # the dual objective carries -h, the primal one +h: their sum is the linear problem's
            lin = model_of(lp, None)
            lin.c = lp.c + d * x                                              # (the same gradient without the term)
            rl = lin.kkt(x, y, omega, *dd)
            h = mo.half(x)
            assert abs((ref["p"] - h) - float(lp.c @ x)) <= 1e-9 * (1 + abs(ref["p"])) and abs((ref["d_adj"] + h) - (rl["d_adj"])) <= 1e-9 * (1 + abs(rl["d_adj"]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("form", ["csr", "tiles"])
def test_kkt_at_the_average_takes_the_pass_without_products(form, dtype):
    """kkt(AVG) after kkt(CUR), flush_average and compute_average reads K'y_avg from the running sums, through the QUAD functor in
    the vector pass: with the y of the averaged iterate overwritten in between, the dual residual is still the one of the TRUE
    average (a pass that multiplied would see the overwritten y), while q'y follows the buffer"""
    lp = get_lp("mid")
    eta, omega, _, _ = steps_of(lp, dtype)
    d = diag_of(lp)
    mo = model_of(lp, d)
    _, _, x1, y1 = start_points(lp, dtype)
    e = lp.engine(dtype, form, quad_diag=dev(d, dtype))
    begin(e, x1, y1, eta, omega)
    e.iterate(40, False)
    e.kkt(N.CUR, omega)
    e.flush_average(False)
    e.compute_average()
    xa, ya = (host(v) for v in e.get_iterate(N.AVG))
    e.buffer(N.BUF_Y_AVG)[:] += 1.0
    got = e.kkt(N.AVG, omega)
    true, moved = mo.kkt(xa, ya, omega), mo.kkt(xa, ya + 1.0, omega)
    rtol, atol = (1e-4, 2e-5) if dtype == torch.float32 else (1e-10, 1e-10)
    assert abs(true["dr"] - moved["dr"]) > 1.0                               # (a product with the overwritten y is far away)
    np.testing.assert_allclose(got["dr"], true["dr"], rtol=rtol, atol=atol)
    np.testing.assert_allclose(got["pr"], true["pr"], rtol=rtol, atol=atol)
    # ... and the same call on a handle whose sums are broken (set_step inside the period) multiplies: it sees the overwritten y
    begin(e, x1, y1, eta, omega)
    e.iterate(20, False)
    e.set_step(float(eta), float(omega), 1.0, 20)
    e.iterate(20, False)
    e.kkt(N.CUR, omega)
    e.flush_average(False)
    e.compute_average()
    xa, ya = (host(v) for v in e.get_iterate(N.AVG))
    e.buffer(N.BUF_Y_AVG)[:] += 1.0
    np.testing.assert_allclose(e.kkt(N.AVG, omega)["dr"], mo.kkt(xa, ya + 1.0, omega)["dr"], rtol=rtol, atol=atol)


# ---------------------------------------------------------------------------------------------------
# 3. all-zero d: the bits of an engine on which the setter was never called
# ---------------------------------------------------------------------------------------------------
ZERO_CASES = [("mid_scaled", f) for f in ("csr", "sorted", "tiles", "tiles_groups")] + [("mid_dense", "tiles_remainder"), ("long", "csr"),
                                                                                       ("long", "tiles_remainder")]


def everything(e, lp, x0, y0, x1, y1, eta, omega):
    """x, y, xbar and the averages after six fixed, six adaptive and six Halpern iterations; the KKT dicts and reports there"""
    out, dicts = [], []
    scaled = lp.d_col is not None
    for adaptive in (False, True):
        begin(e, x1, y1, eta, omega)
        e.iterate(6, adaptive)
        out += list(e.get_iterate(N.CUR)) + [e.buffer(N.BUF_XBAR).clone()]
        dicts.append(e.kkt(N.CUR, omega))
        e.flush_average(adaptive)
        e.compute_average()
        out += list(e.get_iterate(N.AVG))
        for which in (N.AVG, N.PREV, N.CUR):
            for unscaled in ((False, True) if scaled else (False,)):
                dicts.append(e.kkt(which, omega, unscaled=unscaled))
                rep = e.report(which, unscaled=unscaled, omega=omega)
                out += [rep.pop("y"), rep.pop("reduced_costs"), rep.pop("row_activity")]
                dicts.append(rep)
        sc = e.scalars()
        dicts.append({k: sc[k] for k in (sc if adaptive else ("eta", "omega", "tau", "sigma", "eta_sum", "k", "w_pending"))})
    put(e, x0, y0, x1, y1, eta, omega)
    e.halpern_iterate(6)
    out += list(e.get_iterate(N.CUR)) + list(e.get_iterate(N.AVG)) + [e.buffer(N.BUF_XBAR).clone()]
    dicts += [e.kkt(N.AVG, omega), e.kkt(N.CUR, omega)]
    return out, dicts


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name,form", ZERO_CASES, ids=[f"{a}-{b}" for a, b in ZERO_CASES])
def test_all_zero_d_changes_no_bit(name, form, dtype):
    lp = get_lp(name)
    eta, omega, _, _ = steps_of(lp, dtype)
    pts = start_points(lp, dtype)
    plain = lp.engine(dtype, form)
    zero = lp.engine(dtype, form, quad_diag=torch.zeros(lp.n))
    assert plain.quad_diag is None and zero.quad_diag is not None
    (va, da), (vb, db) = everything(plain, lp, *pts, eta, omega), everything(zero, lp, *pts, eta, omega)
    assert len(va) == len(vb) and all(torch.equal(a, b) for a, b in zip(va, vb))
    assert da == db
    # a handle that has worked with a real d, a restart check included, then NULL: the LP's bits again
    d = diag_of(lp)
    zero.set_objective_diag(dev(d, dtype))
    begin(zero, pts[2], pts[3], eta, omega)
    zero.iterate(5, False)
    with_d = zero.get_iterate(N.CUR)[0].clone()
    zero.kkt(N.CUR, omega)
    zero.flush_average(False)
    zero.compute_average()
    zero.kkt(N.AVG, omega)
    zero.restart(N.AVG)
    zero.set_objective_diag(None)
    assert zero.quad_diag is None
    for adaptive in (False, True):
        outs = []
        for e in (plain, zero):
            begin(e, pts[2], pts[3], eta, omega)
            e.iterate(6, adaptive)
            outs.append(list(e.get_iterate(N.CUR)) + [e.buffer(N.BUF_XBAR).clone()])
        assert all(torch.equal(a, b) for a, b in zip(*outs)), adaptive
    begin(plain, pts[2], pts[3], eta, omega)
    plain.iterate(5, False)
    assert not torch.equal(with_d, plain.get_iterate(N.CUR)[0])             # (the real d was at work in between)


# ---------------------------------------------------------------------------------------------------
# 4. together with two-sided rows
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("form", ["csr", "tiles"])
def test_quad_diag_with_q_upper(form, dtype):
    lp = get_lp("mid")
    eta, omega, tau, sigma = steps_of(lp, dtype)
    d = diag_of(lp)
    rng = np.random.default_rng(19)
    x0, _, x1, _ = start_points(lp, dtype)
    y0, y1 = (rng.standard_normal(lp.m).astype(NP[dtype]).astype(np.float64) for _ in range(2))     # (either sign)
    i = np.arange(lp.m)
    qu = np.full(lp.m, INF)
    ineq = i < lp.m_ineq
    qu[ineq & (i % 4 == 1)] = lp.q[ineq & (i % 4 == 1)]
    qu[ineq & (i % 4 >= 2)] = lp.q[ineq & (i % 4 >= 2)] + 0.5
    mo = model_of(lp, d, qu)
    e = lp.engine(dtype, form, quad_diag=dev(d, dtype), q_upper=dev(qu, dtype))
    assert e.quad_diag is not None and e.q_upper is not None
    tol = 3e-5 if dtype == torch.float32 else 1e-11
    begin(e, x1, y1, eta, omega)
    e.iterate(1, False)
    mx, my, _, _ = mo.step(x1, y1, tau, sigma)
    assert (my[:lp.m_ineq] < -0.01).sum() > 10                               # (upper sides are active)
    (xg, yg) = e.get_iterate(N.CUR)
    close(host(xg), mx, tol)
    close(host(yg), my, tol)
    assert_dict(e.kkt(N.CUR, omega), mo.kkt(host(xg), host(yg), omega), dtype, "kkt")
    one_sided = model_of(lp, d).kkt(host(xg), host(yg), omega)
    assert abs(one_sided["pr"] - mo.kkt(host(xg), host(yg), omega)["pr"]) > 1e-2
    begin(e, x1, y1, eta, omega)
    e.iterate(1, True)
    mx, my, me = mo.adaptive_step(x1, y1, float(eta), float(omega), 1)
    (xg, yg) = e.get_iterate(N.CUR)
    close(host(xg), mx, tol)
    close(host(yg), my, tol)
    close([e.scalars()["eta"]], [me], tol)
    put(e, x0, y0, x1, y1, eta, omega)
    e.halpern_iterate(1)
    mx, my, mxc, myc = mo.halpern_step(x1, y1, x0, y0, 0, tau, sigma)
    for got, ref in zip(e.get_iterate(N.CUR) + e.get_iterate(N.AVG), (mx, my, mxc, myc)):
        close(host(got), ref, tol)


# ---------------------------------------------------------------------------------------------------
# 5. state
# ---------------------------------------------------------------------------------------------------
def test_handles_and_calls_without_the_term_are_refused():
    lp = get_lp("edge_free_and_fixed")
    d64 = torch.ones(lp.n, dtype=torch.float64, device=DEV)
    # a mixed-precision handle, in delta mode or not: the library says "call sequence"
    for delta in (True, False):
        em = lp.engine(torch.float32, vec_dtype=torch.float64, delta=delta)
        with pytest.raises(N.PdlpError, match="call sequence"):
            N.check(em.lib.pdlp_set_objective_diag(em.h, d64.data_ptr()), "pdlp_set_objective_diag")
        with pytest.raises(N.PdlpError, match="call sequence"):
            em.set_objective_diag(d64)
        assert em.quad_diag is None
        N.check(em.lib.pdlp_set_objective_diag(em.h, None), "pdlp_set_objective_diag")          # (switching off what is off: fine)
    # a shard of a problem (two ranks in one process; their communicator does nothing)
    from tests.shard_world import World
    w = World(get_lp("mid"), 2, torch.float32, None)
    sh = w.engs[0]
    with pytest.raises(N.PdlpError, match="call sequence"):
        sh.set_objective_diag(torch.ones(sh.nl, dtype=torch.float32, device=DEV))
    assert N.load().pdlp_set_objective_diag(None, None) == -1
    # while it is set: no infeasibility pass, no populations, no batch call; and a malformed vector never reaches the library
    e = lp.engine(torch.float32, quad_diag=torch.ones(lp.n))
    x0, y0, _, _ = start_points(lp, torch.float32)
    begin(e, x0, y0, 0.1, 0.8)
    e.iterate(2, False)
    with pytest.raises(N.PdlpError, match="call sequence"):
        e.detect_infeasibility(1e-4)
    with pytest.raises(N.PdlpError, match="call sequence"):
        e.infeas_reset()
    st, diag = N.C.c_int32(0), (N.C.c_double * 8)()
    assert e.lib.pdlp_infeas_finish(e.h, 1e-4, N.C.byref(st), diag) == e.lib.pdlp_infeas_local(e.h, 1e-4) != 0
    X, Y = torch.zeros(lp.n, 8, device=DEV), torch.zeros(lp.m, 8, device=DEV)
    for call in (lambda: e.mv_steps(X, Y, 1, 0.1, 0.8), lambda: e.mv_gap(X, Y), lambda: e.mv_product(X)):
        with pytest.raises(N.PdlpError, match="call sequence"):
            call()
    for bad in (-torch.ones(lp.n), torch.zeros(lp.n + 1), torch.full((lp.n,), INF)):
        with pytest.raises(ValueError, match="quad_diag"):
            e.set_objective_diag(bad)
    e.set_objective_diag(None)
    e.infeas_reset()
    e.detect_infeasibility(1e-4)
    e.mv_product(X)
    from torchpdlp_amd.batch import BatchEngine
    t = lambda v: dev(v, torch.float32)
    K = tp.CsrPair(lp.m, lp.n, dev(lp.A.indptr, torch.int32), dev(lp.A.indices, torch.int32), t(lp.A.data))
    be = BatchEngine(K, lp.m_ineq, t(lp.c), t(lp.q), t(lp.l), t(lp.u), 2)
    V = torch.ones(lp.n, be.Bp, device=DEV)
    be.product(V)
    be.eng.set_objective_diag(torch.ones(lp.n))
    with pytest.raises(N.PdlpError, match="call sequence"):
        be.product(V)
    be.eng.set_objective_diag(None)
    be.product(V)


def test_setting_d_drops_the_captured_graphs():
    lp = get_lp("mid")
    dtype = torch.float32
    eta, omega, tau, sigma = steps_of(lp, dtype)
    d = diag_of(lp)
    _, _, x1, y1 = start_points(lp, dtype)
    e = lp.engine(dtype, "csr")
    e.set_option(N.OPT_GRAPH, 1)
    begin(e, x1, y1, eta, omega)
    e.iterate(11, False)                       # a captured segment of the LP ...
    e.iterate(11, False)                       # ... replayed
    lin = model_of(lp, None)
    mx, my = x1, y1
    for _ in range(22):
        mx, my, _, _ = lin.step(mx, my, tau, sigma)
    tol = 3e-5 * 22 / 6                        # (what six steps are granted, grown linearly: the operator is non-expansive)
    close(host(e.get_iterate(N.CUR)[0]), mx, tol)
    e.set_objective_diag(dev(d, dtype))
    begin(e, x1, y1, eta, omega)
    e.iterate(11, False)                       # the same segment length: a stale graph would replay the LP's functors
    e.iterate(11, False)
    mo = model_of(lp, d)
    qx, qy = x1, y1
    for _ in range(22):
        qx, qy, _, _ = mo.step(qx, qy, tau, sigma)
    xg, yg = e.get_iterate(N.CUR)
    close(host(xg), qx, tol)
    close(host(yg), qy, tol)
    assert np.max(np.abs(qx - mx)) > 0.05      # (the two results are far apart)
    # graph replay against direct launches with the term: the same bits
    f = lp.engine(dtype, "csr", quad_diag=dev(d, dtype))
    begin(f, x1, y1, eta, omega)
    f.iterate(11, False)
    f.iterate(11, False)
    assert all(torch.equal(a, b) for a, b in zip(f.get_iterate(N.CUR), (xg, yg)))


# ---------------------------------------------------------------------------------------------------
# 6. whole solves of problems with a constructed optimum (seeds checked on the float64 model: solved in under 1100 iterations in
#    every mode)
# ---------------------------------------------------------------------------------------------------
SOLVES = {"plain": dict(adaptive_stepsize=True), "fixed": {}, "ruiz_pc": dict(precondition=True, pock_chambolle=True),
          "halpern": dict(halpern=True), "q_upper": dict(adaptive_stepsize=True)}
SIZES = {"37x23": (37, 23, 1, None), "600x520_tiled": (600, 520, 1, 8)}
_QPS = {}


def qp_of(size):
    if size not in _QPS:
        m, n, seed, per_row = SIZES[size]
        _QPS[size] = make_qp(m, n, seed, per_row=per_row)
    return _QPS[size]


def solve_and_check(qp, dtype, tol, mode):
    t = lambda v: dev(v, dtype)
    kw = dict(SOLVES[mode])
    if mode == "q_upper":       # upper sides that the optimum respects (x* stays optimal): K x* + 1 on every third inequality row
        qu = np.where((np.arange(qp.m) < qp.m_ineq) & (np.arange(qp.m) % 3 == 0), qp.A @ qp.xs + 1.0, INF)
        kw["q_upper"] = t(qu)
    problem = (t(qp.c), tp.CsrPair.from_any(qp.A, device=DEV, dtype=dtype), t(qp.q), qp.m_ineq, t(qp.l), t(qp.u))
    res = tp.solve_lp(problem, tol=tol, dtype=dtype, seed=3, primal_weight_update=True, quad_diag=t(qp.d), **kw)
    print(f"{qp.m} x {qp.n} {mode} tol {tol:g}: k={res.iterations} n={res.restarts} j={res.kkt_passes} objective {res.objective:.10g} "
          f"(opt {qp.opt:.10g}) dual {res.dual_objective:.10g} rel {res.rel_primal_residual:.3g} {res.rel_dual_residual:.3g} {res.rel_gap:.3g}")
    assert res.status == "Solved", (res.status, res.iterations)
    bound = 1e-3 * (1 + abs(qp.opt)) if tol == 1e-4 else 2e-8 * (1 + 2 * abs(qp.opt))
    assert abs(res.objective - qp.opt) <= bound, (res.objective, qp.opt)
    assert max(res.rel_primal_residual, res.rel_dual_residual, res.rel_gap) <= tol, \
        (res.rel_primal_residual, res.rel_dual_residual, res.rel_gap)
    x = host(res.x).reshape(-1)
    eps = 4 * float(np.finfo(NP[dtype]).eps) if "precondition" in kw else 0.0       # (un-scaled x: the rounding of D_col * (l / D_col))
    lo, hi = qp.l.copy(), qp.u.copy()
    lo[np.isfinite(lo)] -= eps * np.abs(lo[np.isfinite(lo)])
    hi[np.isfinite(hi)] += eps * np.abs(hi[np.isfinite(hi)])
    assert (x >= lo).all() and (x <= hi).all()
    assert abs(float(qp.c @ x + 0.5 * np.sum(qp.d * x * x)) - res.objective) <= 1e-2
    assert abs(float(qp.c @ x) - qp.opt) > 10 * bound                                      # (and c'x alone is another number)
    return res


@pytest.mark.parametrize("mode", list(SOLVES))
def test_solve_qp_37x23(mode):
    solve_and_check(qp_of("37x23"), torch.float32, 1e-4, mode)


@pytest.mark.parametrize("mode", list(SOLVES))
def test_solve_qp_37x23_float64(mode):
    solve_and_check(qp_of("37x23"), torch.float64, 1e-8, mode)


@pytest.mark.parametrize("mode", list(SOLVES))
def test_solve_qp_tiled_600x520(mode, monkeypatch):
    """PDLP_TILED=1 with 64-column panels puts both products of the solve's engine on k_tiled_fused"""
    monkeypatch.setenv("PDLP_TILED", "1")
    monkeypatch.setenv("PDLP_TILE_LW", "6")
    qp = qp_of("600x520_tiled")
    t = lambda v: dev(v, torch.float32)
    eng = tp.PdlpEngine.from_full(tp.CsrPair.from_any(qp.A, device=DEV, dtype=torch.float32), t(qp.c), t(qp.q), t(qp.l), t(qp.u), qp.m_ineq,
                                  quad_diag=t(qp.d))
    assert all(k.startswith("tiled") for k in eng.kernels), eng.kernels
    del eng
    solve_and_check(qp, torch.float32, 1e-4, mode)
