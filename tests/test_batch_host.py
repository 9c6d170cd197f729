"""CPU checks of the batched solves and of the host-side rules they share with the single-LP solver (torchpdlp_amd/rules.py): the
rules on arrays and on scalars against scalar transcriptions of the reference kept here, the pdlp_batch struct against the header,
argument validation before any device work, and gen_lp_family's stated optima."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import torchpdlp_amd as tp
from torchpdlp_amd import _native as N
from torchpdlp_amd import rules
from torchpdlp_amd.batch import batch_decisions, kkt_finish, termination
from torchpdlp_amd.solver import check_termination, kkt_from_residuals, primal_weight_from_distances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scalar_decision(kc, ka, kp, kf, tt, k, j, live, max_kkt, t=np.float32):
    """the loop of oracle.pdlp_algorithm for one LP (pdhg.py:115-146, :67)"""
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


def scalar_residuals(red, t):
    """helpers.py:84-96 for one LP from the six sums of a KKT pass (PDLP_BUF_RED order), every value rounded to t"""
    dr, lp, un, p, pr, d = (float(v) for v in red)
    adj = t(t(t(d) + t(lp)) + t(un))
    return dict(pr=t(np.sqrt(pr)), dr=t(np.sqrt(dr)), gap=t(adj - t(p)), p=t(p), d_adj=adj)


def scalar_kkt_error(pr, dr, gap, omega, t):
    """KKT_error (helpers.py:98-108) for one LP, every intermediate rounded to t"""
    w2 = t(t(omega) * t(omega))
    s = t(t(w2 * t(t(pr) * t(pr))) + t(t(t(dr) * t(dr)) / w2))
    return t(np.sqrt(t(s + t(t(gap) * t(gap)))))


def scalar_terminated(pr, dr, gap, p, d_adj, q_norm, c_norm, tol, t):
    """check_termination (helpers.py:110-128) for one LP; the gap is signed"""
    eps, one = t(tol), t(1)
    return bool(t(pr) <= t(eps * t(one + t(q_norm))) and t(dr) <= t(eps * t(one + t(c_norm)))
                and t(gap) <= t(eps * t(t(one + t(abs(p))) + t(abs(d_adj)))))


def is_scalar(v):
    return isinstance(v, np.generic)


def test_the_earlier_names_are_the_rules():
    assert batch_decisions is rules.restart_decision and kkt_finish is rules.kkt_from_sums and termination is rules.terminated
    assert kkt_from_residuals is rules.kkt_error and primal_weight_from_distances is rules.primal_weight
    assert (tp.STATUS_SOLVED, tp.STATUS_KKT_LIMIT, tp.STATUS_TIME_LIMIT) == (rules.STATUS_SOLVED, rules.STATUS_KKT_LIMIT,
                                                                             rules.STATUS_TIME_LIMIT)


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
        want = (2 if use_avg else 1) if crit >= 0 else (1 if capped else 0)
        # the same LP as one of an array, and alone: numpy scalars and 0-d arrays in, numpy scalars out
        d0 = rules.restart_decision(kc[i], ka[i], kp[i], kf[i], tt[i], k[i], j[i], live[i], max_kkt, t)
        d1 = rules.restart_decision(*(np.asarray(a[i]) for a in (kc, ka, kp, kf, tt, k, j, live)), max_kkt, t)
        assert all(is_scalar(v) for v in (*d0.values(), *d1.values())), i
        for got in ({key: v[i] for key, v in d.items()}, d0, d1):
            assert got["crit"] == crit, i
            assert not live[i] or bool(got["use_avg"]) == use_avg, i
            assert bool(got["capped"]) == capped, i
            assert got["action"] == want, i
        # what PdhgDriver asks: whether KKT_previous can matter, and the decision without a pass cap
        if live[i]:
            lazy = rules.restart_decision(kc[i], ka[i], kp[i] if rules.previous_kkt_matters(kc[i], ka[i], kf[i], t) else t(np.inf),
                                          kf[i], int(tt[i]), int(k[i]), int(j[i]), live=True, t=t)
            assert (lazy["crit"], bool(lazy["use_avg"]), bool(lazy["capped"])) == (crit, use_avg, False), i
    assert (d["action"][~live] == 0).all()
    assert d["action"].dtype == np.int32


def test_kkt_finish_and_termination_match_the_scalar_rules():
    for t in (np.float32, np.float64):
        rng = np.random.default_rng(1)
        B = 4000
        red = np.abs(rng.standard_normal((B, 6))) * rng.choice([1e-8, 1e-3, 1.0, 1e3], (B, 6))
        red[:, 1:4] *= rng.choice([-1, 1], (B, 3))
        omega = rng.uniform(0.1, 10, B).astype(t)
        r = kkt_finish(red, omega, t)
        qn, cn = rng.uniform(0, 10, B).astype(t), rng.uniform(0, 10, B).astype(t)
        term = termination(r, qn, cn, 1e-4, t)
        omega2 = rng.uniform(0.1, 10, B).astype(t)                   # the residuals under another primal weight (pdhg.py:153)
        again = rules.kkt_error(r, omega2, t)
        assert all(v.dtype == t for v in (*r.values(), again)) and term.dtype == bool
        for i in range(B):
            want = scalar_residuals(red[i], t)
            want["kkt"] = scalar_kkt_error(want["pr"], want["dr"], want["gap"], omega[i], t)
            r0 = rules.kkt_from_sums(red[i], omega[i], t)                # one LP alone
            for key in want:
                assert r[key][i] == want[key] and r0[key] == want[key], (i, key)
                assert is_scalar(r0[key]) and r0[key].dtype == t, (i, key)
            res = {key: float(r[key][i]) for key in r}                   # as the engine hands them to PdhgDriver: Python floats
            assert r["kkt"][i] == kkt_from_residuals(res, omega[i], t)
            k2 = scalar_kkt_error(want["pr"], want["dr"], want["gap"], omega2[i], t)
            assert again[i] == k2 and rules.kkt_error(res, omega2[i], t) == k2 and is_scalar(rules.kkt_error(res, omega2[i], t)), i
            done = scalar_terminated(want["pr"], want["dr"], want["gap"], want["p"], want["d_adj"], qn[i], cn[i], 1e-4, t)
            t0 = rules.terminated(res, qn[i], cn[i], 1e-4, t)
            assert bool(term[i]) == done and bool(t0) == done and is_scalar(t0), i
            assert done == check_termination(r["pr"][i], r["dr"][i], r["gap"][i], r["p"][i], r["d_adj"][i], qn[i], cn[i], t(1e-4))
        assert term.any() and not term.all()


@pytest.mark.parametrize("t", [np.float32, np.float64])
def test_start_values_on_arrays_and_scalars(t):
    qn = np.array([0.0, 1e-7, 2.0, 3.0, 5e-7], t)
    cn = np.array([1.0, 4.0, 1e-9, 6.0, 0.0], t)
    w = rules.start_omega(qn, cn, t)
    assert w.dtype == t and w.tolist() == [1.0, 1.0, 1.0, 2.0, 1.0]               # pdhg.py:23: 1 unless both norms exceed 1e-6
    for i in range(len(qn)):
        w0 = rules.start_omega(qn[i], cn[i], t)
        assert is_scalar(w0) and w0.dtype == t and w0 == w[i]
    eta = rules.start_eta(3.7, t)
    assert is_scalar(eta) and eta.dtype == t and eta == t(0.9) / t(3.7)           # pdhg.py:22


@pytest.mark.parametrize("t", [np.float32, np.float64])
def test_primal_weight_of_an_array_is_its_elements_one_by_one(t):
    rng = np.random.default_rng(2)
    B = 3000
    dx2, dy2 = rng.uniform(0, 50, B) * rng.choice([0.0, 1e-12, 1.0, 1e6], B), rng.uniform(0, 50, B) * rng.choice([0.0, 1e-9, 1.0], B)
    omega = (rng.uniform(0.01, 100, B) * rng.choice([1e-3, 1.0, 1e3], B)).astype(t)
    w = rules.primal_weight(dx2, dy2, omega, 0.5, t)
    assert w.dtype == t and w.shape == (B,)
    one = [rules.primal_weight(float(dx2[i]), float(dy2[i]), omega[i], 0.5, t) for i in range(B)]
    assert all(is_scalar(v) and v.dtype == t for v in one)
    assert w.tobytes() == np.array(one, t).tobytes()
    assert (w[(dx2 == 0) | (dy2 == 0)] == omega[(dx2 == 0) | (dy2 == 0)]).all()       # enhancements.py:78: no move, no update
    assert (w != omega).any()


def test_rules_module_needs_neither_torch_nor_the_native_library():
    """torchpdlp_amd/rules.py is plain numpy: importing it pulls in neither torch nor the HIP library.  (The package's __init__
    imports torch for the solver entry points, so the fresh interpreter gets the package folder without its __init__.)"""
    code = """
import sys, types
pkg = types.ModuleType("torchpdlp_amd")
pkg.__path__ = [sys.argv[1]]
sys.modules["torchpdlp_amd"] = pkg
import torchpdlp_amd.rules as rules
assert rules.BETA == (0.2, 0.8, 0.36) and rules.STATUS_SOLVED == "Solved"
assert float(rules.kkt_error(dict(pr=3.0, dr=4.0, gap=0.0), 1.0)) == 5.0
loaded = [m for m in sys.modules if m == "torch" or m.startswith("torch.") or m.startswith("torchpdlp_amd.") and m != "torchpdlp_amd.rules"]
assert not loaded, loaded
assert "libpdlp_hip" not in open("/proc/self/maps").read()
"""
    done = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "torchpdlp_amd")], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr


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
