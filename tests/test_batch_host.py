"""CPU checks of the batched solves: the vectorised restart decisions against the scalar rules, the pdlp_batch struct against the
header, argument validation before any device work, and gen_lp_family's stated optima."""
import os
import re

import numpy as np
import pytest
import torch

import torchpdlp_amd as tp
from torchpdlp_amd import _native as N
from torchpdlp_amd.batch import batch_decisions, kkt_finish, termination
from torchpdlp_amd.solver import check_termination, kkt_from_residuals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scalar_decision(kc, ka, kp, kf, tt, k, j, live, max_kkt, t=np.float32):
    """the loop of oracle.pdlp_algorithm / PdhgDriver.advance for one LP (pdhg.py:115-146, :67)"""
    if not live:
        return -1, False, False
    k_min = min(kc, ka)
    crit = -1
    if k_min <= t(0.2) * kf:
        crit = 0
    elif k_min <= t(0.8) * kf and k_min > kp:
        crit = 1
    elif tt >= 0.36 * k:
        crit = 2
    return crit, bool(kc >= ka), crit < 0 and j >= max_kkt


@pytest.mark.parametrize("t", [np.float32, np.float64])
def test_batch_decisions_match_the_scalar_rules(t):
    rng = np.random.default_rng(0)
    B = 4000
    kc = rng.choice([0.5, 1.0, 2.0], B).astype(t) * rng.uniform(0.5, 1.5, B).astype(t)
    ka = np.where(rng.random(B) < 0.2, kc, rng.uniform(0.1, 2.0, B).astype(t)).astype(t)     # ties included
    kp = np.where(rng.random(B) < 0.2, np.minimum(kc, ka), rng.uniform(0.1, 2.0, B).astype(t)).astype(t)
    kf = np.where(rng.random(B) < 0.3, t(0), rng.uniform(0.1, 5.0, B).astype(t)).astype(t)      # KKT_first = 0: first check
    k = rng.integers(1, 50, B) * 40
    tt = np.minimum(rng.integers(1, 20, B) * 40, k)
    j = rng.integers(100, 300, B)
    live = rng.random(B) < 0.8
    max_kkt = 250
    d = batch_decisions(kc, ka, kp, kf, tt, k, j, live, max_kkt, t)
    for i in range(B):
        crit, use_avg, capped = scalar_decision(kc[i], ka[i], kp[i], kf[i], tt[i], k[i], j[i], live[i], max_kkt, t)
        assert d["crit"][i] == crit, i
        assert not live[i] or bool(d["use_avg"][i]) == use_avg, i
        assert bool(d["capped"][i]) == capped, i
        want = (2 if use_avg else 1) if crit >= 0 else (1 if capped else 0)
        assert d["action"][i] == want, i
    assert (d["action"][~live] == 0).all()


def test_kkt_finish_and_termination_match_the_scalar_rules():
    rng = np.random.default_rng(1)
    B = 500
    red = np.abs(rng.standard_normal((B, 6))) * rng.choice([1e-8, 1e-3, 1.0, 1e3], (B, 6))
    red[:, 1:4] *= rng.choice([-1, 1], (B, 3))
    omega = rng.uniform(0.1, 10, B).astype(np.float32)
    r = kkt_finish(red, omega)
    qn, cn = rng.uniform(0, 10, B).astype(np.float32), rng.uniform(0, 10, B).astype(np.float32)
    term = termination(r, qn, cn, 1e-4)
    for i in range(B):
        res = {key: float(r[key][i]) for key in r}
        assert r["kkt"][i] == kkt_from_residuals(res, omega[i])
        assert bool(term[i]) == check_termination(r["pr"][i], r["dr"][i], r["gap"][i], r["p"][i], r["d_adj"][i], qn[i], cn[i],
                                                  np.float32(1e-4))


def test_batch_struct_matches_header():
    src = open(os.path.join(ROOT, "include", "pdlp_hip.h")).read()
    body = re.search(r"typedef struct pdlp_batch \{(.*?)\} pdlp_batch;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [d.strip().split()[-1].lstrip("*") for d in decl.split(",")]
    assert names == [f[0] for f in N.PdlpBatch._fields_]
    assert N.BATCH_PART_PER_COL == 2 * 4 * 8192 and "(2 * 4 * 8192)" in src
    assert "pdlp_batch_iterate" in N.SIGNATURES and N.ABI_VERSION == 18


def test_batch_entry_points_reject_nonsense_without_a_gpu():
    import ctypes as C
    lib = N.load()
    b = N.PdlpBatch()
    assert lib.pdlp_batch_iterate(None, C.byref(b), 1, 0, 0) == -1
    assert lib.pdlp_batch_kkt(None, C.byref(b), 0, 0, 0) == -1
    assert lib.pdlp_batch_kkt(None, C.byref(b), 5, 0, 0) == -1
    assert lib.pdlp_batch_restart(None, C.byref(b), 3) == -1
    assert lib.pdlp_batch_average(None, None, 0) == -1


def small_problem(B=3):
    f = tp.gen_lp_family(30, 20, 3, B, seed=1)
    K = tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val)
    return f, (f.C[:, 0], K, f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0])


@pytest.mark.parametrize("flag", [dict(comm=True), dict(fishnet=True), dict(precision="mixed"), dict(infeasibility_detect=True),
                                  dict(adaptive_retry=True), dict(direct_exchange=True)])
def test_unsupported_flags_raise_before_device_work(flag, monkeypatch):
    f, prob = small_problem()
    monkeypatch.setattr(tp.batch, "BatchEngine", None)          # any device work would fail differently
    with pytest.raises(ValueError):
        tp.solve_lp_batch(prob, f.C, device="cpu", **flag)


def test_shapes_are_validated_before_device_work(monkeypatch):
    f, prob = small_problem()
    monkeypatch.setattr(tp.batch, "BatchEngine", None)
    with pytest.raises(ValueError, match="disagree"):
        tp.solve_lp_batch(prob, f.C, f.Q[:, :2], device="cpu")
    with pytest.raises(ValueError, match="shape"):
        tp.solve_lp_batch(prob, f.C[:-1], device="cpu")
    with pytest.raises(ValueError, match="shape"):
        tp.solve_lp_batch(prob, q=f.Q.unsqueeze(0), device="cpu")
    with pytest.raises(ValueError, match="shape"):
        tp.solve_lp_batch(prob, x_init=torch.zeros(f.n + 1), device="cpu")
    with pytest.raises(ValueError, match="columns"):
        tp.solve_lp_batch(prob, f.C, x_init=torch.zeros(f.n, f.B + 1), device="cpu")
    with pytest.raises(ValueError, match="columns"):
        tp.solve_lp_batch(prob, q=f.Q, y_init=torch.zeros(f.m, 2), device="cpu")
    with pytest.raises(ValueError, match="columns"):
        tp.solve_lp_batch(os.path.join(ROOT, "tests", "golden", "mps", "afiro.mps"), x_init=torch.zeros(32, 2), device="cpu")
    with pytest.raises(ValueError):
        tp.solve_lp_batch(prob, f.C, device="cpu", dtype=torch.float16)


def test_gen_lp_family_optima_satisfy_kkt():
    f = tp.gen_lp_family(60, 45, 4, 5, seed=2, dtype=torch.float64)
    K = torch.sparse_csr_tensor(f.rowptr, f.colidx.long(), f.val, (f.m, f.n)).to_dense().numpy()
    for b in range(f.B):
        x, y = f.X_opt[:, b].numpy(), f.Y_opt[:, b].numpy()
        c, q, l, u = (v[:, b].numpy() for v in (f.C, f.Q, f.L, f.U))
        r = K @ x - q
        assert (r[:f.m_ineq] >= -1e-9).all() and np.abs(r[f.m_ineq:]).max() < 1e-9         # primal feasible
        assert (x >= l - 1e-12).all() and (x <= u + 1e-12).all()
        assert (y[:f.m_ineq] >= 0).all() and np.abs(y[:f.m_ineq] * r[:f.m_ineq]).max() < 1e-9
        lam = c - K.T @ y                                                                    # reduced costs
        at_l, at_u = np.isclose(x, l), np.isclose(x, u)
        assert (np.abs(lam[~at_l & ~at_u]) < 1e-9).all()
        assert (lam[at_l & ~at_u] >= -1e-9).all() and (lam[at_u & ~at_l] <= 1e-9).all()
        assert abs(float(c @ x) - f.opt_obj[b]) < 1e-9 * (1 + abs(f.opt_obj[b]))


def test_gen_lp_family_agrees_with_highs():
    opt = pytest.importorskip("scipy.optimize")
    f = tp.gen_lp_family(40, 30, 4, 4, seed=3, dtype=torch.float64)
    K = torch.sparse_csr_tensor(f.rowptr, f.colidx.long(), f.val, (f.m, f.n)).to_dense().numpy()
    for b in range(f.B):
        c, q, l, u = (v[:, b].numpy() for v in (f.C, f.Q, f.L, f.U))
        bounds = [(None if np.isinf(a) else a, None if np.isinf(z) else z) for a, z in zip(l, u)]
        h = opt.linprog(c, A_ub=-K[:f.m_ineq], b_ub=-q[:f.m_ineq], A_eq=K[f.m_ineq:], b_eq=q[f.m_ineq:], bounds=bounds, method="highs")
        assert h.status == 0
        assert abs(h.fun - f.opt_obj[b]) <= 1e-6 * (1 + abs(f.opt_obj[b]))
