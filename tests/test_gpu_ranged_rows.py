"""Two-sided constraint rows q <= K x <= q_upper on the GPU (pdlp_set_row_upper, PdlpEngine(q_upper=), solve_lp(q_upper=)):
all-infinite q_upper against an engine without it bit for bit, six iterations (fixed, adaptive, Halpern) against the float64 numpy
model of tests/ranged_model.py through every product form, the KKT and report sums against the model within the running-error
bounds of tests/test_gpu_report.py, whole solves against the split twin, and the handle's state around the new call."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import torchpdlp_amd as tp
from tests.conftest import GOLDEN
from tests.host_lp import DEV, NP, get_lp
from tests.ranged_model import RangedModel, feasible_ranged_lp
from tests.test_gpu_halpern import SCENARIOS, close, host, put, start_points
from tests.test_gpu_report import C_BOUND, U64, assert_within, build_engine, h64, make_lp, raw_report, ref_report
from torchpdlp_amd import _native as N
from torchpdlp_amd.ranged import split_rows

RANGED = os.path.join(GOLDEN, "ranged", "ranged.mps")
DTYPES = [torch.float32, torch.float64]
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _setup():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    N.load()


def dev(v, dtype):
    return torch.tensor(np.asarray(v), dtype=dtype, device=DEV)


def f32(v):
    return np.asarray(v, np.float32).astype(np.float64)


def model_of(lp, qu):
    return RangedModel(lp.A, lp.m_ineq, lp.c, lp.q, lp.l, lp.u, qu)


# ---------------------------------------------------------------------------------------------------
# 1. all-infinite q_upper: the bits of an engine that has none
# ---------------------------------------------------------------------------------------------------
def everything(e, lp, dtype, x0, y0, x1, y1, eta, omega):
    """iterates after 6 fixed, 6 adaptive and 6 Halpern iterations, KKT dicts at CUR / AVG / PREV (scaled and un-scaled), reports"""
    out, dicts = [], []
    for adaptive in (False, True):
        e.set_iterate(dev(x1, dtype), dev(y1, dtype))
        e.set_step(eta, omega, 1.0, 0)
        e.iterate(6, adaptive)
        out += list(e.get_iterate(N.CUR))
        dicts.append(e.kkt(N.CUR, omega))
        e.flush_average(adaptive)
        e.compute_average()
        out += list(e.get_iterate(N.AVG))
        for which in (N.AVG, N.PREV, N.CUR):
            for unscaled in (False, True):
                dicts.append(e.kkt(which, omega, unscaled=unscaled))
                rep = e.report(which, unscaled=unscaled, omega=omega)
                out += [rep.pop("y"), rep.pop("reduced_costs"), rep.pop("row_activity")]
                dicts.append(rep)
        sc = e.scalars()          # (the step-size rule's own scalars only mean something after an adaptive iteration)
        dicts.append({k: sc[k] for k in (sc if adaptive else ("eta", "omega", "tau", "sigma", "eta_sum", "k", "w_pending"))})
    put(e, x0, y0, x1, y1, eta, omega)
    e.halpern_iterate(6)
    out += list(e.get_iterate(N.CUR)) + list(e.get_iterate(N.AVG))
    dicts += [e.kkt(N.AVG, omega), e.kkt(N.CUR, omega, unscaled=True), e.report(N.AVG, unscaled=True, omega=omega)]
    out += [dicts[-1].pop(k) for k in ("y", "reduced_costs", "row_activity")]
    return out, dicts


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("form", ["csr", "tiles", "tiles_groups"])
def test_all_infinite_q_upper_changes_no_bit(form, dtype):
    lp = get_lp("mid_scaled")
    eta, omega = 0.9 / lp.norm2(), 0.8
    pts = start_points(lp, dtype)
    plain = lp.engine(dtype, form)
    ranged = lp.engine(dtype, form, q_upper=torch.full((lp.m,), INF))
    assert plain.q_upper is None and ranged.q_upper is not None
    (va, da), (vb, db) = everything(plain, lp, dtype, *pts, eta, omega), everything(ranged, lp, dtype, *pts, eta, omega)
    assert len(va) == len(vb) and all(torch.equal(a, b) for a, b in zip(va, vb))
    assert da == db


# ---------------------------------------------------------------------------------------------------
# 2. six iterations against the numpy model
# ---------------------------------------------------------------------------------------------------
def sided_q_upper(lp, x1, y1, tau, sigma):
    """q_upper for the step from (x1, y1): the inequality rows cycle through (q, +inf), (q, q) and two kinds of (q, q_upper) with a
    gap.  On the rows with a gap: where a = y + sigma (q - k) > 0 the lower side is active whatever q_upper is; where a < 0, with
    z = k - y / sigma > q, q_upper = (q + z) / 2 < z makes b = a / 2 < 0 (the upper side is active) and q_upper = 2z - q + 1 > z
    makes b > 0 (neither).  Every value is a float32 number >= q."""
    base = model_of(lp, None)
    _, _, _, k = base.step(x1, y1, tau, sigma)
    a = y1 + sigma * (lp.q - k)
    z = k - y1 / sigma
    i = np.arange(lp.m)
    qu = np.full(lp.m, INF)
    ineq = i < lp.m_ineq
    qu[ineq & (i % 4 == 1)] = lp.q[ineq & (i % 4 == 1)]
    gap = ineq & (i % 4 >= 2)
    qu[gap] = lp.q[gap] + 1.0
    up, none = gap & (a < 0) & (i % 4 == 2), gap & (a < 0) & (i % 4 == 3)
    qu[up] = 0.5 * (lp.q[up] + z[up])
    qu[none] = 2 * z[none] - lp.q[none] + 1.0
    qu = f32(qu)
    assert (qu[ineq] >= lp.q[ineq]).all()
    return qu


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name,form", SCENARIOS, ids=[f"{a}-{b}" for a, b in SCENARIOS])
def test_six_iterations_against_the_model(name, form, dtype):
    lp = get_lp(name)
    eta, omega = 0.9 / lp.norm2(), 0.8
    T = NP[dtype]
    tau, sigma = float(T(eta) / T(omega)), float(T(eta) * T(omega))         # (as k_set_step rounds them)
    rng = np.random.default_rng(17)
    x0, _, x1, _ = start_points(lp, dtype)
    y0, y1 = (rng.standard_normal(lp.m).astype(T) for _ in range(2))        # (either sign: a two-sided row's y may be negative)
    x0, x1, y0, y1 = (v.astype(np.float64) for v in (x0, x1, y0, y1))
    qu = sided_q_upper(lp, x1, y1, tau, sigma)
    mo = model_of(lp, qu)
    _, _, _, k = mo.step(x1, y1, tau, sigma)
    lower, upper, neither = (int(v.sum()) for v in mo.sides(y1, k, sigma))
    print(f"{name}: {lp.m_ineq} inequality rows; first step: lower side active on {lower}, upper on {upper}, neither on {neither}")
    if lp.m_ineq >= 12:            # (every LP of the list but the one without inequality rows and the 1 x 1)
        assert lower > 0 and upper > 0 and neither > 0
        assert (qu[:lp.m_ineq] == lp.q[:lp.m_ineq]).any() and np.isinf(qu[:lp.m_ineq]).any()
    e = lp.engine(dtype, form, q_upper=dev(qu, dtype))
    # the tolerance test_gpu_halpern.py grants its six-iteration model comparison in the same precision
    tol = 3e-5 if dtype == torch.float32 else 1e-11
    # fixed step
    e.set_iterate(dev(x1, dtype), dev(y1, dtype))
    e.set_step(eta, omega, 1.0, 0)
    e.iterate(6, False)
    mx, my = x1, y1
    for _ in range(6):
        mx, my, _, _ = mo.step(mx, my, tau, sigma)
    xg, yg = e.get_iterate(N.CUR)
    close(host(xg), mx, tol)
    close(host(yg), my, tol)
    if lp.m_ineq >= 12:            # an implementation that reads q_upper as +inf would be far off: some y stay below zero
        assert (my[:lp.m_ineq] < -10 * tol).any() and (host(yg)[:lp.m_ineq] < 0).any()
    # adaptive step (one trial per iteration, kept when rejected; k counts from 1 as in __graft_entry__.smoke)
    e.set_iterate(dev(x1, dtype), dev(y1, dtype))
    e.set_step(eta, omega, 1.0, 0)
    e.iterate(6, True)
    mx, my, me = x1, y1, float(eta)
    for it in range(1, 7):
        mx, my, me = mo.adaptive_step(mx, my, me, float(omega), it)
    xg, yg = e.get_iterate(N.CUR)
    close(host(xg), mx, tol)
    close(host(yg), my, tol)
    # Halpern: anchor (x0, y0), iterate (x1, y1)
    put(e, x0.astype(T), y0.astype(T), x1.astype(T), y1.astype(T), eta, omega)
    e.halpern_iterate(6)
    mx, my = x1, y1
    for it in range(6):
        mx, my, mxc, myc = mo.halpern_step(mx, my, x0, y0, it, tau, sigma)
    (xg, yg), (xc, yc) = e.get_iterate(N.CUR), e.get_iterate(N.AVG)
    for got, ref in ((xg, mx), (yg, my), (xc, mxc), (yc, myc)):
        close(host(got), ref, tol)


# ---------------------------------------------------------------------------------------------------
# 3. KKT and report sums against the model
# ---------------------------------------------------------------------------------------------------
def ref_ranged_rows(P, qu, x, y, unscaled, u):
    """the constraint side of tests/test_gpu_report.py:ref_report with both sides of a row: (act, sums[2]) and their bounds, built
    the same way (a product's error, u times the size of every rounded result, factor 1 through the projections, the double sums)"""
    m = P.m
    ineq = np.arange(m) < P.m_ineq
    two = ineq & np.isfinite(qu)
    quf = np.where(two, qu, 0.0)
    kx, e_kx = P.K @ x, (P.Lr + 1) * u * (P.Ka @ np.abs(x))
    rr, ru = kx - P.q, kx - quf
    e_rr, e_ru = e_kx + u * np.abs(rr), e_kx + u * np.abs(ru)
    qi, qs, yi, act, e_act = P.q, quf, y, kx, e_kx
    e_q = e_qs = e_y = np.zeros(m)
    if unscaled:
        d = P.drow
        rr, ru = rr / d, ru / d
        e_rr, e_ru = e_rr / d + u * np.abs(rr), e_ru / d + u * np.abs(ru)
        qi, qs, yi, act = P.q / d, quf / d, y * d, kx / d
        e_q, e_qs, e_y, e_act = u * np.abs(qi), u * np.abs(qs), u * np.abs(yi), e_kx / d + u * np.abs(act)
    lower = np.where(ineq & (rr > 0), 0.0, rr)
    upper = np.where(two, np.maximum(ru, 0.0), 0.0)
    e_up = np.where(two, e_ru, 0.0)
    dsum = lambda terms: (len(terms) + 2) * U64 * np.abs(terms).sum()
    sq = np.concatenate([lower * lower, upper * upper])
    s, b = np.zeros(2), np.zeros(2)
    s[0] = sq.sum()
    b[0] = (2 * np.abs(lower) * e_rr + e_rr ** 2).sum() + (2 * np.abs(upper) * e_up + e_up ** 2).sum() + dsum(sq)
    up_side = two & (y < 0)
    side, e_side = np.where(up_side, qs, qi), np.where(up_side, e_qs, e_q)
    s[1] = (side * yi).sum()
    b[1] = (e_side * np.abs(yi) + e_y * np.abs(side) + e_side * e_y).sum() + dsum(side * yi)
    return act, e_act, s, b, int((upper > 0).sum()), int(up_side.sum())


@pytest.mark.parametrize("family", ["csr", "sorted", "tiled"])
@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_kkt_and_report_sums_against_the_model(T, family):
    rng = np.random.default_rng(23)
    P = make_lp(T, rng, m_ineq=400)
    eng = build_engine(P, family)
    # a random point; sides around K x so that upper sides are violated, and negative y on two-sided rows
    x0 = np.clip(rng.uniform(-1.5, 1.5, P.n), P.l, P.u).astype(T).astype(np.float64)
    y0 = rng.uniform(-1, 1, P.m).astype(T).astype(np.float64)
    kx = P.K @ x0
    i = np.arange(P.m)
    ineq = i < P.m_ineq
    qu = np.full(P.m, INF)
    qu[ineq & (i % 4 == 1)] = P.q[ineq & (i % 4 == 1)]
    gap = ineq & (i % 4 >= 2)
    qu[gap] = np.where(kx[gap] > P.q[gap], P.q[gap] + 0.5 * (kx[gap] - P.q[gap]), P.q[gap] + 1.0)
    qu = np.asarray(qu, T).astype(np.float64)
    y0[ineq & np.isinf(qu)] = np.abs(y0[ineq & np.isinf(qu)])
    TT = torch.float32 if T is np.float32 else torch.float64
    eng.set_row_upper(dev(qu, TT))
    eng.set_iterate(dev(x0, TT), dev(y0, TT))
    eng.set_step(0.05, 1.3, 1.0, 0)
    eng.iterate(3, False)
    eng.flush_average(False)
    eng.compute_average()
    mo = RangedModel(P.K, P.m_ineq, P.c, P.q, P.l, P.u, qu)
    u = np.finfo(T).eps
    for which in (N.CUR, N.AVG, N.PREV):
        x, y = (h64(v) for v in eng.get_iterate(which))
        for unscaled in (0, 1):
            lam, _, s6, e_lam, _, b6 = ref_report(P, x, y, unscaled, u)
            act, e_act, s2, b2, n_up, n_neg = ref_ranged_rows(P, qu, x, y, unscaled, u)
            assert n_up > 10 and n_neg > 10, (n_up, n_neg)             # violated upper sides and negative y on two-sided rows
            want, bound = np.concatenate([s6[:4], s2]), np.concatenate([b6[:4], b2])
            # the bounded reference and the few-line model agree (two statements of the same sums)
            r = mo.kkt(x, y, 1.0, *((P.dcol, P.drow) if unscaled else (None, None)))
            assert abs(r["pr"] ** 2 - s2[0]) <= 1e-9 * (1 + s2[0]) and abs(r["d_adj"] - (s2[1] + s6[1] + s6[2])) <= 1e-9 * (1 + np.abs(want).sum())
            tag = f"which={which} unscaled={unscaled}"
            rc_d, act_d, red = raw_report(eng, which, unscaled)
            assert_within(h64(rc_d), lam, e_lam, f"reduced costs {tag}")
            assert_within(h64(act_d), act, e_act, f"row activity {tag}")
            assert_within(red, want, bound, f"report sums {tag}")
            _, _, red_a = raw_report(eng, which, unscaled, want_rc=False, want_act=False)
            assert_within(red_a, want, bound, f"report sums without stores {tag}")
            N.check(eng.lib.pdlp_kkt_local(eng.h, which, unscaled), "pdlp_kkt_local")
            red_k = (N.C.c_double * N.NRED)()
            N.check(eng.lib.pdlp_read_red(eng.h, red_k), "pdlp_read_red")
            assert_within(np.array(red_k[:6]), want, bound, f"pdlp_kkt_local's sums {tag}")
            # read as +inf the sums would be the one-sided ones: far outside the bound
            assert abs(s2[0] - s6[4]) > 100 * C_BOUND * b2[0] and abs(s2[1] - s6[5]) > 100 * C_BOUND * b2[1]


# ---------------------------------------------------------------------------------------------------
# 4. whole solves: the native form against its split twin
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twins():
    A, m_ineq, c, q, l, u, qu = feasible_ranged_lp(160, 120, 4, seed=4)
    As, qs, mi, _ = split_rows(A, q, qu, m_ineq)
    return (A, m_ineq, c, q, l, u, qu), (As, mi, qs)


def residuals64(A, m_ineq, c, q, l, u, qu, x, y, q_norm, c_norm):
    """the three relative residuals of the two-sided LP at (x, y) in float64 numpy"""
    r = RangedModel(A, m_ineq, c, q, l, u, qu).kkt(x, y, 1.0)
    return r["pr"] / (1 + q_norm), r["dr"] / (1 + c_norm), r["gap"] / (1 + abs(r["p"]) + abs(r["d_adj"])), r


def two_sided_norm(q, qu, m_ineq):
    two = (np.arange(q.size) < m_ineq) & np.isfinite(qu)
    return float(np.linalg.norm(np.where(two, np.maximum(np.abs(q), np.abs(qu)), q)))


SOLVES = {"plain": dict(adaptive_stepsize=True), "ruiz_pc": dict(precondition=True, pock_chambolle=True), "halpern": dict(halpern=True)}


@pytest.mark.parametrize("prec", ["f32_1e-4", "f64_1e-8"])
@pytest.mark.parametrize("mode", list(SOLVES))
def test_solve_lp_native_against_split(twins, mode, prec):
    (A, m_ineq, c, q, l, u, qu), (As, mi, qs) = twins
    dtype, tol = (torch.float32, 1e-4) if prec == "f32_1e-4" else (torch.float64, 1e-8)
    kw = dict(tol=tol, dtype=dtype, seed=3, primal_weight_update=True, max_kkt=2_000_000, **SOLVES[mode])
    t = lambda v: dev(v, dtype)
    native = tp.solve_lp((t(c), tp.CsrPair.from_any(A, device=DEV, dtype=dtype), t(q), m_ineq, t(l), t(u)), q_upper=t(qu), **kw)
    split = tp.solve_lp((t(c), tp.CsrPair.from_any(As, device=DEV, dtype=dtype), t(qs), mi, t(l), t(u)), **kw)
    assert native.status == "Solved" == split.status, (native.status, split.status)
    x, y = h64(native.x), h64(native.y)
    eps = 4 * float(np.finfo(NP[dtype]).eps) if "precondition" in kw else 0.0       # (un-scaled x: the rounding of D_col * (l / D_col))
    ub = u.copy()
    ub[np.isfinite(u)] += eps * np.abs(u[np.isfinite(u)])
    assert (x >= l - eps * np.abs(l)).all() and (x <= ub).all()
    # the norms the termination test was given: of q (two-sided) and c, of the scaled problem when preconditioned
    q_norm, c_norm = two_sided_norm(q, qu, m_ineq), float(np.linalg.norm(c))
    if "precondition" in kw:
        _, sc = tp.equilibrate_matrix(tp.CsrPair.from_any(A, device=DEV, dtype=dtype), DEV, pock_chambolle=True)
        cs, qss, _, _, qus = sc.scale(t(c), t(q), t(l), t(u), t(qu))
        q_norm, c_norm = two_sided_norm(h64(qss), h64(qus), m_ineq), float(np.linalg.norm(h64(cs)))
    rp, rd, rg, r = residuals64(A, m_ineq, c, q, l, u, qu, x, y, q_norm, c_norm)
    print(f"{mode} {prec}: native k={native.iterations} split k={split.iterations}; objective {native.objective:.10g} / "
          f"{split.objective:.10g}; recomputed rel. residuals {rp:.3g} {rd:.3g} {rg:.3g} (library: {native.rel_primal_residual:.3g} "
          f"{native.rel_dual_residual:.3g} {native.rel_gap:.3g}); y < 0 on {int((y[:m_ineq] < 0).sum())} rows")
    assert max(rp, rd, rg) <= tol, (rp, rd, rg)
    assert abs(native.objective - split.objective) <= 2 * tol * (1 + abs(r["p"]) + abs(r["d_adj"])), (native.objective, split.objective)
    assert (y[:m_ineq][np.isinf(qu[:m_ineq])] >= 0).all()
    assert (y[:m_ineq] < 0).any()                       # an active upper side: the LP is built to have some


@pytest.mark.parametrize("prec", ["f32_1e-4", "f64_1e-8"])
def test_solve_lp_ranged_mps(prec):
    dtype, tol = (torch.float32, 1e-4) if prec == "f32_1e-4" else (torch.float64, 1e-8)
    kw = dict(tol=tol, dtype=dtype, seed=3, primal_weight_update=True, max_kkt=2_000_000)
    native, split = tp.solve_lp(RANGED, ranged_rows=True, **kw), tp.solve_lp(RANGED, **kw)
    assert native.status == "Solved" == split.status
    c, K, q, m_ineq, l, u, qu = tp.mps_to_ranged_form(RANGED, dtype=torch.float64)
    import scipy.sparse as sp
    A = sp.csr_matrix((K.val.numpy(), K.colidx.numpy(), K.rowptr.numpy()), shape=(K.m, K.n))
    c, q, l, u, qu = (h64(v) for v in (c, q, l, u, qu))
    x, y = h64(native.x), h64(native.y)
    assert native.y.shape == (12, 1) and split.y.shape == (16, 1)
    assert (x >= l).all() and (x <= u).all()
    rp, rd, rg, r = residuals64(A, m_ineq, c, q, l, u, qu, x, y, two_sided_norm(q, qu, m_ineq), float(np.linalg.norm(c)))
    print(f"ranged.mps {prec}: native k={native.iterations} split k={split.iterations}; objective {native.objective:.10g} / "
          f"{split.objective:.10g}; recomputed rel. residuals {rp:.3g} {rd:.3g} {rg:.3g}")
    assert max(rp, rd, rg) <= tol, (rp, rd, rg)
    assert abs(native.objective - split.objective) <= 2 * tol * (1 + abs(r["p"]) + abs(r["d_adj"]))


# ---------------------------------------------------------------------------------------------------
# 5. state
# ---------------------------------------------------------------------------------------------------
def test_graph_replay_gives_the_bits_of_direct_launches():
    lp = get_lp("mid")
    eta, omega, dtype = 0.9 / lp.norm2(), 0.8, torch.float32
    x0, y0, x1, y1 = start_points(lp, dtype)
    tau, sigma = float(np.float32(eta) / np.float32(omega)), float(np.float32(eta) * np.float32(omega))
    qu = sided_q_upper(lp, x1.astype(np.float64), y1.astype(np.float64), tau, sigma)
    outs = []
    for graph in (False, True):
        e = lp.engine(dtype, "csr", q_upper=dev(qu, dtype))
        if graph:
            e.set_option(N.OPT_GRAPH, 1)
        res = []
        for adaptive in (False, True):
            e.set_iterate(dev(x1, dtype), dev(y1, dtype))
            e.set_step(eta, omega, 1.0, 0)
            e.iterate(11, adaptive)
            e.iterate(8, adaptive)
            res += list(e.get_iterate(N.CUR)) + [torch.tensor([e.scalars()[k] for k in ("eta", "eta_sum", "k")])]
        if graph:        # switching the rows off drops the captured graphs: the next replay runs the one-sided functors
            e.set_row_upper(None)
            e.set_iterate(dev(x1, dtype), dev(y1, dtype))
            e.set_step(eta, omega, 1.0, 0)
            e.iterate(11, False)
            p = lp.engine(dtype, "csr")
            p.set_iterate(dev(x1, dtype), dev(y1, dtype))
            p.set_step(eta, omega, 1.0, 0)
            p.iterate(11, False)
            assert all(torch.equal(a, b) for a, b in zip(e.get_iterate(N.CUR), p.get_iterate(N.CUR)))
            assert not torch.equal(res[1], p.get_iterate(N.CUR)[1])
        outs.append(res)
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert (outs[0][1][:lp.m_ineq] < 0).any()           # (two-sided rows were at work)


@pytest.mark.parametrize("form", ["csr", "tiles"])
def test_null_returns_the_handle_to_one_sided_rows(form):
    lp = get_lp("mid_scaled")
    eta, omega, dtype = 0.9 / lp.norm2(), 0.8, torch.float64
    pts = start_points(lp, dtype)
    x1, y1 = pts[2].astype(np.float64), pts[3].astype(np.float64)
    qu = sided_q_upper(lp, x1, y1, eta / omega, eta * omega)
    plain, e = lp.engine(dtype, form), lp.engine(dtype, form, q_upper=dev(qu, dtype))
    # the handle works with two-sided rows first, a restart check included (products kept by KKT passes, running sums) ...
    e.set_iterate(dev(x1, dtype), dev(y1, dtype))
    e.set_step(eta, omega, 1.0, 0)
    e.iterate(5, False)
    e.kkt(N.CUR, omega)
    e.flush_average(False)
    e.compute_average()
    with_rows = e.kkt(N.AVG, omega)
    e.restart(N.AVG)
    # ... a null pointer in the middle of it: the K'y kept by the pass and the candidates' products are dropped, nothing else is needed
    e.set_row_upper(None)
    assert e.q_upper is None
    va, da = everything(plain, lp, dtype, *pts, eta, omega)
    vb, db = everything(e, lp, dtype, *pts, eta, omega)
    assert all(torch.equal(a, b) for a, b in zip(va, vb)) and da == db
    # and back on, on the used handle: the bits of a fresh engine with the rows
    e.set_row_upper(dev(qu, dtype))
    fresh = lp.engine(dtype, form, q_upper=dev(qu, dtype))
    va, da = everything(fresh, lp, dtype, *pts, eta, omega)
    vb, db = everything(e, lp, dtype, *pts, eta, omega)
    assert all(torch.equal(a, b) for a, b in zip(va, vb)) and da == db
    assert with_rows["pr"] > 0


def test_handles_and_calls_without_two_sided_rows_are_refused():
    lp = get_lp("edge_free_and_fixed")
    qu64 = torch.full((lp.m,), INF, dtype=torch.float64, device=DEV)
    # a mixed-precision handle, in delta mode or not: the library says "call sequence", the engine ValueError before it asks
    for delta in (True, False):
        em = lp.engine(torch.float32, vec_dtype=torch.float64, delta=delta)
        with pytest.raises(N.PdlpError, match="call sequence"):
            N.check(em.lib.pdlp_set_row_upper(em.h, qu64.data_ptr()), "pdlp_set_row_upper")
        with pytest.raises(ValueError, match="q_upper"):
            em.set_row_upper(qu64)
        N.check(em.lib.pdlp_set_row_upper(em.h, None), "pdlp_set_row_upper")          # (switching off what is off: fine)
    # a shard of a problem (two ranks in one process; their communicator does nothing)
    from tests.shard_world import World
    w = World(get_lp("mid"), 2, torch.float32, None)
    sh = w.engs[0]
    qs = torch.full((sh.ml,), INF, dtype=torch.float32, device=DEV)
    with pytest.raises(N.PdlpError, match="call sequence"):
        N.check(sh.lib.pdlp_set_row_upper(sh.h, qs.data_ptr()), "pdlp_set_row_upper")
    with pytest.raises(ValueError, match="q_upper"):
        sh.set_row_upper(qs)
    assert N.load().pdlp_set_row_upper(None, None) == -1
    # while it is set: no infeasibility pass, no populations, no delta mode; and a malformed vector never reaches the library
    e = lp.engine(torch.float32, q_upper=torch.full((lp.m,), INF))
    x0, y0, _, _ = start_points(lp, torch.float32)
    e.set_iterate(dev(x0, torch.float32), dev(y0, torch.float32))
    e.set_step(0.1, 0.8, 1.0, 0)
    e.iterate(2, False)
    with pytest.raises(N.PdlpError, match="call sequence"):
        e.detect_infeasibility(1e-4)
    X, Y = torch.zeros(lp.n, 8, device=DEV), torch.zeros(lp.m, 8, device=DEV)
    for call in (lambda: e.mv_steps(X, Y, 1, 0.1, 0.8), lambda: e.mv_gap(X, Y), lambda: e.mv_product(X)):
        with pytest.raises(N.PdlpError, match="call sequence"):
            call()
    bad = torch.full((lp.m,), INF)
    bad[0] = float(lp.q[0]) - 1.0
    with pytest.raises(ValueError, match="q_upper"):
        e.set_row_upper(bad)
    with pytest.raises(ValueError):
        e.set_row_upper(torch.zeros(lp.m + 1))
    e.set_row_upper(None)
    e.detect_infeasibility(1e-4)
    e.mv_product(X)
