"""``tests/population_model.py`` is pinned before it judges the population kernels: in float64 its step and gap are the oracle's
per column, in float32 arithmetic it reproduces the reference's recorded first fishnet round, its bounds are neither vacuous nor too
tight (the same operation in the working precision with every row's items in reverse order stays inside them).  No GPU."""
import functools

import numpy as np
import pytest

from tests import population_model as pm
from tests import test_gpu_batch_kernels as bk

C_BOUND, SHAPES = bk.C_BOUND, bk.SHAPES
CASES = SHAPES + ["mixed_400x300"]
TYPES = pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
J = 8
OMEGA, THETA = 1.3, 1.0


@functools.lru_cache(maxsize=None)
def lp_of(case, T):
    rng = np.random.default_rng(CASES.index(case))
    if case == "mixed_400x300":
        return bk.golden_lp(T, 1, rng, per="cqlu")[0]
    return bk.shape_lp(case, T, 1, "cqlu", rng)


def start(case, T):
    P = lp_of(case, T)
    X, Y = pm.draw_population(P, J, np.random.default_rng(50 + CASES.index(case)))
    return P, X, Y, bk.eta_base(P)


@pytest.mark.parametrize("case", CASES)
def test_step_and_gap_are_the_oracles(case):
    """float64 on both sides, another order of the sums: within the model's own float64 bound"""
    T, u = np.float64, bk.units(np.float64)
    P, X, Y, eta = start(case, T)
    o = P.oracle(0)
    X1, Y1, ex, ey = pm.steps(P, X, Y, 1, eta, OMEGA, THETA, T, u)
    X3, Y3, ex3, ey3 = pm.steps(P, X, Y, 3, eta, OMEGA, THETA, T, u)
    gap, eg = pm.gap(P, X1, Y1, T, u)
    for p in range(J):
        xo, yo = o.step_fixed(X[:, p], Y[:, p], eta, OMEGA, THETA)
        bk.close(f"{case} column {p} x", X1[:, p], xo, ex[:, p])
        bk.close(f"{case} column {p} y", Y1[:, p], yo, ey[:, p])
        bk.close(f"{case} column {p} gap", gap[p], float(o.kkt(X1[:, p], Y1[:, p], OMEGA)["gap"]), eg[p])
        for _ in range(2):
            xo, yo = o.step_fixed(xo, yo, eta, OMEGA, THETA)
        bk.close(f"{case} column {p} x after 3 steps", X3[:, p], xo, ex3[:, p])
        bk.close(f"{case} column {p} y after 3 steps", Y3[:, p], yo, ey3[:, p])
    assert np.abs(X1 - X).max() > 0 or case == "1x1"
    if P.m_ineq:
        assert (Y1[:P.m_ineq] == 0).any() and (Y1[:P.m_ineq] > 0).any(), "the projection must act on some rows and not on others"


def test_float32_arithmetic_reproduces_the_recorded_round(golden):
    """the reference's first fishnet round (tests/golden/fishnet.npz): K pts0, k steps per point, the gaps, in float32"""
    T = np.float32
    g = golden("fishnet.npz")
    for name in ("mixed_400x300", "box_200x150", "mixed_27x32"):
        r = g.group(name)
        P = bk.golden_lp(T, 1, np.random.default_rng(0), per="cqlu", file="fishnet.npz", name=name)[0]
        X = r["pts0"]
        Y, _ = pm.product(P, X, arith=T)
        X, Y, _, _ = pm.steps(P, X, Y, int(r["k"]), float(r["eta"]), float(r["omega"]), 1.0, T, arith=T)
        gaps, _ = pm.gap(P, X, Y, T, arith=T)
        ref = g.group(f"{name}/round0")["gaps"]
        scale = float(np.max(np.abs(ref))) + 1e-30
        np.testing.assert_allclose(gaps, ref, rtol=3e-4, atol=3e-4 * scale, err_msg=name)      # test_fishnet_vs_reference_golden's


def outputs(case, T, **kw):
    """every operation once -> {name: (value, bound or None, scale)}"""
    P, X, Y, eta = start(case, T)
    u = None if kw else bk.units(T)
    rng = np.random.default_rng(7)
    out = {}
    kx, e = pm.product(P, X, u, **kw)
    out["product"] = (kx, e)
    for k in (1, 3):
        xs, ys, ex, ey = pm.steps(P, X, Y, k, eta, OMEGA, THETA, T, u, **kw)
        out[f"steps{k} x"], out[f"steps{k} y"] = (xs, ex), (ys, ey)
    S, E, sizes = pm.gap_terms(P, X, Y, u, **kw)
    out["gap sums"] = (S, E)
    out["gap"] = pm.gap_from_terms(S, T, E, u)
    W = rng.uniform(0, 1, (J, 5))
    W = (W / W.sum(0)).astype(T)
    out["combine"] = pm.combine(X, W, u, **kw)
    scales = {k: float(np.abs(np.asarray(v, np.float64)).max()) for k, (v, _) in out.items()}
    scales["gap sums"] = scales["gap"] = float(sizes.sum(0).max())        # sums that cancel: the size of what is added
    return out, scales


@TYPES
@pytest.mark.parametrize("case", CASES)
def test_bounds_are_not_vacuous(case, T):
    out, scales = outputs(case, T)
    lim = 1e-3 if T == np.float32 else 1e-11
    for name, (v, e) in out.items():
        assert np.isfinite(e).all() and (e >= 0).all(), name
        assert e.max() == 0 or e.max() < lim * scales[name], (name, float(e.max()), scales[name])


@TYPES
@pytest.mark.parametrize("case", CASES)
def test_bounds_hold_for_another_order(case, T):
    """the working precision, every row's items (and every sum's terms) in reverse order: inside C_BOUND times the bound"""
    out, _ = outputs(case, T)
    other, _ = outputs(case, T, arith=T, reverse=True)
    moved = 0
    for name, (v, e) in out.items():
        w = np.asarray(other[name][0], np.float64)
        bk.close(f"{case} {name}", w, v, e)
        moved += int((w != np.asarray(v, np.float64)).sum())
    assert moved or case == "1x1", "the other order must round differently somewhere"
