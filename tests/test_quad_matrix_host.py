"""The sparse quadratic objective c'x + 1/2 x'Qx on the host (no GPU): the validation of ``quad_matrix`` and every refusal before
device work, the step rule ``rules.qp_eta``, the scaling rule ``Q_s = D_col Q D_col``, and ``run_pdlp`` over a float64 numpy engine
that implements the linearised step (tests/qp_model.py) on problems with a constructed optimum -- the instances of the issue's table."""
import numpy as np
import pytest
import torch

import torchpdlp_amd as tp
from tests.qp_model import GeneralQuadEngine, GeneralQuadModel, make_general_qp, model_of_general_qp, quad_matrix_of
from tests.quad_model import QuadModelEngine, model_of_qp, make_qp
from torchpdlp_amd import _native as N
from torchpdlp_amd.compose import QMAT_REFUSED, check_composition
from torchpdlp_amd.quad import check_quad_matrix
from torchpdlp_amd.rules import qp_eta, start_eta
from torchpdlp_amd.solver import estimate_quad_norm, pdlp_algorithm, run_pdlp

INF = float("inf")
K3 = torch.eye(3)
V3 = torch.zeros(3)
Q3 = torch.tensor([[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 0.0]])
NAN = float("nan")
BAD = {"not_square": torch.ones(3, 2), "wrong_size": torch.eye(4), "value_asymmetry": torch.tensor([[2.0, 1.0, 0.0], [0.5, 2.0, 0.0], [0.0, 0.0, 1.0]]),
       "pattern_asymmetry": torch.tensor([[2.0, 1.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 1.0]]),
       "negative_diagonal": torch.tensor([[2.0, 1.0, 0.0], [1.0, -2.0, 0.0], [0.0, 0.0, 1.0]]),
       "nan": torch.tensor([[2.0, NAN, 0.0], [NAN, 2.0, 0.0], [0.0, 0.0, 1.0]]), "inf": torch.tensor([[INF, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 1.0]])}


# ---------------------------------------------------------------------------------------------------
# 1. validation and refusals, all before device work
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BAD))
def test_malformed_quad_matrix_raises_before_any_device_work(name):
    with pytest.raises(ValueError, match="quad_matrix"):
        check_quad_matrix(BAD[name], 3)
    with pytest.raises(ValueError, match="quad_matrix"):
        pdlp_algorithm(K3, 2, V3, V3, V3, V3 + 1, "cpu", verbose=False, quad_matrix=BAD[name])
    with pytest.raises(ValueError, match="quad_matrix"):
        tp.solve_lp((V3, K3, V3, 2, V3, V3 + 1), device="cpu", quad_matrix=BAD[name])


def test_well_formed_quad_matrix_passes_the_check():
    import scipy.sparse as sp
    for ok in (Q3, Q3.double(), Q3.to_sparse(), sp.csr_matrix(Q3.numpy()), tp.CsrPair.from_any(Q3), torch.zeros(3, 3)):
        out = check_quad_matrix(ok, 3)
        assert isinstance(out, tp.CsrPair) and out.shape == (3, 3)
    assert check_quad_matrix(None, 3) is None
    assert check_quad_matrix(Q3, None).nnz == 4
    # ... and then reaches the device: on a machine without one, or with device="cpu", that is the first failure
    with pytest.raises(Exception) as e:
        tp.solve_lp((V3, K3, V3, 2, V3, V3 + 1), device="cpu", quad_matrix=Q3)
    assert not isinstance(e.value, ValueError)


REFUSALS = [dict(adaptive=True), dict(halpern=True), dict(adaptive=True, adaptive_retry=True), dict(infeasibility_detect=True),
            dict(precision="mixed"), dict(comm=True), dict(direct_exchange=True), dict(fishnet=True)]


@pytest.mark.parametrize("kw", REFUSALS, ids=lambda kw: "+".join(kw))
def test_refused_combinations_raise_before_any_device_work(kw):
    names = dict(adaptive="adaptive_stepsize")
    with pytest.raises(ValueError, match="quad_matrix") as e:
        tp.solve_lp((V3, K3, V3, 2, V3, V3 + 1), device="cpu", quad_matrix=Q3, **{names.get(k, k): v for k, v in kw.items()})
    assert str(e.value) == QMAT_REFUSED
    if not ({"fishnet", "direct_exchange"} & set(kw)):                    # (these two are solve_lp's flags)
        with pytest.raises(ValueError, match="quad_matrix") as e:
            pdlp_algorithm(K3, 2, V3, V3, V3, V3 + 1, "cpu", verbose=False, quad_matrix=Q3, **kw)
        assert str(e.value) == QMAT_REFUSED
    rule = {("mixed" if k == "precision" else k): True for k in kw}
    with pytest.raises(ValueError) as e:
        check_composition(quad_matrix=True, **rule)
    assert str(e.value) == QMAT_REFUSED
    # the switches it composes with are not refused
    check_composition(quad_matrix=True, quad_diag=True, q_upper=True)


def test_the_batch_refuses_and_a_path_is_checked_before_it_is_read():
    with pytest.raises(ValueError, match="quad_matrix"):
        tp.solve_lp_batch((V3, K3, V3, 2, V3, V3 + 1), device="cpu", quad_matrix=Q3)
    for bad in ("not_square", "value_asymmetry", "pattern_asymmetry", "negative_diagonal", "nan"):
        with pytest.raises(ValueError, match="quad_matrix"):
            tp.solve_lp("no/such/file.mps", device="cpu", quad_matrix=BAD[bad])
    with pytest.raises(Exception) as e:
        tp.solve_lp("no/such/file.mps", device="cpu", quad_matrix=Q3)
    assert not isinstance(e.value, ValueError)


def test_driver_refuses_too():
    """run_pdlp / PdhgDriver over an engine that has quad_matrix: the same refusals, before the engine is used"""
    class Engine:
        comm, mixed, delta, q_upper, quad_diag, quad_matrix, m_ineq = None, False, False, None, None, Q3, 1
        dtype = torch.float32

        def __getattr__(self, name):
            raise AssertionError(f"engine.{name} was used")
    for kw in (dict(adaptive=True), dict(halpern=True), dict(infeasibility_detect=True), dict(adaptive=True, adaptive_retry=True)):
        with pytest.raises(ValueError, match="quad_matrix"):
            run_pdlp(Engine(), verbose=False, sigma=1.0, **kw)

    class Mixed(Engine):
        mixed = True
    with pytest.raises(ValueError, match="quad_matrix"):
        run_pdlp(Mixed(), verbose=False, sigma=1.0)


def test_library_entry_points():
    lib = N.load()
    for name in ("pdlp_objective_matrix_bytes", "pdlp_set_objective_matrix", "pdlp_objective_product"):
        assert name in N.SIGNATURES
    assert N.ABI_VERSION == 18 == lib.pdlp_abi_version()
    assert lib.pdlp_set_objective_matrix(None, None, None, None, None, 0) == -1
    assert lib.pdlp_objective_product(None, None, None) == -1
    assert lib.pdlp_objective_matrix_bytes(None, 0, None) == -1


# ---------------------------------------------------------------------------------------------------
# 2. the step rule
# ---------------------------------------------------------------------------------------------------
GRID = [(s, L, w) for s in (1e-3, 0.37, 1.0, 7.5, 4e3) for L in (1e-6, 0.02, 1.0, 33.0, 1e5) for w in (1e-4, 0.05, 1.0, 12.0, 3e3)]


def test_qp_eta_is_start_eta_without_a_matrix():
    for t in (np.float32, np.float64):
        for s in (1e-3, 0.37, 1.0, 7.5, 4e3):
            for w in (1e-4, 1.0, 3e3):
                a, b = qp_eta(s, 0.0, w, t), start_eta(s, t)
                assert type(a) is type(b) is t and a == b


@pytest.mark.parametrize("t", [np.float32, np.float64], ids=["f32", "f64"])
def test_qp_eta_satisfies_the_step_condition_and_is_rounded_once(t):
    for s, L, w in GRID:
        eta = qp_eta(s, L, w, t)
        assert type(eta) is t and eta > 0
        e = np.float64(eta)
        # omega/eta - eta omega s^2 >= L/2, with room: at 0.9 of the root the left side is above 1.11 times the right (or the
        # K term alone decides: L/2 is negligible, and eta is 0.9 / s up to rounding)
        lhs, rhs = w / e - e * w * s * s, L / 2
        assert lhs >= 1.11 * rhs, (s, L, w, lhs, rhs)
        assert e <= 0.9 / s * (1 + 1e-6)
        # rounded once: the double formula, then one conversion
        # (the root (-L/2 + sqrt(L^2/4 + 4 w^2 s^2)) / (2 w s^2) written with its conjugate, which does not cancel for large L)
        root = 2.0 * w / (0.5 * L + np.sqrt(0.25 * L * L + 4.0 * w * w * s * s))
        assert abs(np.float64(eta) - 0.9 * root) <= (0.5000001 * np.spacing(t(0.9 * root)) if t is np.float32 else 4 * np.spacing(0.9 * root))
        if L <= 1e3 * w * s:                                                 # where the plain form is still accurate, it agrees
            plain = (-0.5 * L + np.sqrt(0.25 * L * L + 4.0 * w * w * s * s)) / (2.0 * w * s * s)
            assert abs(plain - root) <= 1e-8 * root
        # and it is 0.9 of the largest admissible step: the condition fails just above eta / 0.9
        big = 1.001 * e / 0.9
        assert w / big - big * w * s * s < rhs * (1 + 1e-9) + 1e-300 or rhs < 1e-12 * w / big


# ---------------------------------------------------------------------------------------------------
# 3. the scaling rule
# ---------------------------------------------------------------------------------------------------
def test_scaling_returns_d_col_q_d_col_and_keeps_it_symmetric():
    rng = np.random.default_rng(5)
    n = 60
    Q = quad_matrix_of(n, 2, "lowrank")
    dc = rng.uniform(0.3, 3.0, n)
    s = tp.Scaling(torch.from_numpy(dc), torch.ones(4, dtype=torch.float64))
    c, q, l, u = torch.ones(n, dtype=torch.float64), torch.ones(4, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.ones(n, dtype=torch.float64)
    four, five = s.scale(c, q, l, u), s.scale(c, q, l, u, quad_matrix=Q)
    seven = s.scale(c, q, l, u, q, c, Q)
    assert len(four) == 4 and len(five) == 5 and len(seven) == 7
    assert all(torch.equal(a, b) for a, b in zip(four, five))
    for Qs in (five[4], seven[6]):
        assert isinstance(Qs, tp.CsrPair)
        check_quad_matrix(Qs, n)                                         # symmetric bit for bit: the engine's own check passes
        np.testing.assert_allclose(Qs.to_dense().numpy(), dc[:, None] * Q.toarray() * dc[None, :], rtol=1e-15, atol=0)
    # 1/2 x'Qx is invariant: x = D_col x_s
    x = rng.standard_normal(n)
    xs = x / dc
    assert abs(x @ (Q @ x) - xs @ (five[4].to_dense().numpy() @ xs)) <= 1e-12 * abs(x @ (Q @ x))


def test_half_and_unscaled_kkt_are_invariant_under_the_scaling():
    qp = make_general_qp(40, 60, 2, kind="lowrank", diag=True)
    rng = np.random.default_rng(2)
    dc, dr = rng.uniform(0.5, 2.0, qp.n), rng.uniform(0.5, 2.0, qp.m)
    A, Q = qp.A.toarray(), qp.Q.toarray()
    orig = GeneralQuadModel(A, qp.m_ineq, qp.c, qp.q, qp.l, qp.u, Q, qp.d)
    scaled = GeneralQuadModel(dr[:, None] * A * dc[None, :], qp.m_ineq, qp.c * dc, qp.q * dr, qp.l / dc, qp.u / dc,
                              Q * (dc[:, None] * dc[None, :]), qp.d * dc * dc)
    x, y = rng.standard_normal(qp.n), rng.standard_normal(qp.m)
    rel = lambda a, b: abs(a - b) / max(abs(a), abs(b), 1e-300)
    assert orig.half(x) > 1.0 and rel(orig.half(x), scaled.half(x / dc)) <= 1e-12
    want, got = orig.kkt(x, y, 0.7), scaled.kkt(x / dc, y / dr, 0.7, dc, dr)
    for key in want:
        assert rel(want[key], got[key]) <= 1e-11, (key, want[key], got[key])
    # the slots: [3] - h is c'x and [1] + h is l'lam+ of the LP with the same gradient
    sw, _ = orig.sums(x, y)
    lin = GeneralQuadModel(A, qp.m_ineq, qp.c + Q @ x + qp.d * x, qp.q, qp.l, qp.u).sums(x, y)[0]
    h = orig.half(x)
    assert rel(sw[3] - h, qp.c @ x) <= 1e-12 and rel(sw[1] + h, lin[1]) <= 1e-12 and sw[0] == lin[0] and sw[2] == lin[2]


# ---------------------------------------------------------------------------------------------------
# 4. run_pdlp over the numpy engine: the instances of the issue's table
# ---------------------------------------------------------------------------------------------------
def bound_of(tol, opt):
    """the objective bound of tests/test_gpu_quad.py"""
    return 1e-3 * (1 + abs(opt)) if tol == 1e-4 else 2e-8 * (1 + 2 * abs(opt))


TABLE = {"37x23_lowrank_1e-8": (37, 23, None, "lowrank", 1e-8), "37x23_lowrank_1e-4": (37, 23, None, "lowrank", 1e-4),
         "600x520_sparse_1e-4": (600, 520, 8, "sparse", 1e-4), "300x2600_arrow_1e-4": (300, 2600, 6, "arrow", 1e-4)}


@pytest.mark.parametrize("case", list(TABLE))
def test_run_pdlp_solves_the_instances_of_the_table(case):
    m, n, per_row, kind, tol = TABLE[case]
    qp = make_general_qp(m, n, 1, per_row, kind)
    mo = model_of_general_qp(qp)
    assert abs(mo.objective(qp.xs) - qp.opt) <= 1e-12 * (1 + abs(qp.opt)) and qp.Q.nnz > 0
    x, obj, k, nr, j, status, _ = run_pdlp(GeneralQuadEngine(mo), tol=tol, verbose=False, primal_update=True, seed=3)
    print(f"{case}: k={k} n={nr} j={j} objective {obj:.12g} (opt {qp.opt:.12g})")
    assert status == "Solved", (status, k)
    assert abs(obj - qp.opt) <= bound_of(tol, qp.opt), (obj, qp.opt)
    xv = x.numpy()
    assert (xv >= qp.l).all() and (xv <= qp.u).all()
    assert abs(obj - mo.objective(xv)) <= 1e-9 * (1 + abs(obj))
    assert abs(float(qp.c @ xv) - qp.opt) > 10 * bound_of(tol, qp.opt)        # (c'x alone is another number: the term is at work)


def ruiz_pock_chambolle(A, sweeps=20):
    """Ruiz sweeps and one Pock-Chambolle pass (alpha = 1) in numpy -> (D_col, D_row) with A_s = D_row A D_col"""
    A = np.abs(A).astype(np.float64)
    dc, dr = np.ones(A.shape[1]), np.ones(A.shape[0])
    nz = lambda v: np.where(v > 0, v, 1.0)
    for _ in range(sweeps):
        r, c = np.sqrt(nz(A.max(1))), np.sqrt(nz(A.max(0)))
        A, dr, dc = A / r[:, None] / c[None, :], dr / r, dc / c
    r, c = np.sqrt(nz(A.sum(1))), np.sqrt(nz(A.sum(0)))
    return dc / c, dr / r


def test_run_pdlp_with_ruiz_and_pock_chambolle():
    """the scaled problem (Scaling.scale with quad_matrix) on the numpy engine; the termination test and the objective are those of
    the original problem (the un-scaled KKT pass)"""
    tol = 1e-8
    qp = make_general_qp(37, 23, 1, None, "lowrank")
    dc, dr = ruiz_pock_chambolle(qp.A.toarray())
    s = tp.Scaling(torch.from_numpy(dc), torch.from_numpy(dr))
    cs, qs, ls, us, Qs = s.scale(*(torch.from_numpy(v) for v in (qp.c, qp.q, qp.l, qp.u)), quad_matrix=qp.Q)
    As = dr[:, None] * qp.A.toarray() * dc[None, :]
    mo = GeneralQuadModel(As, qp.m_ineq, cs.numpy(), qs.numpy(), ls.numpy(), us.numpy(), Qs.to_dense().numpy())
    eng = GeneralQuadEngine(mo, scaling=(dc, dr))
    x, obj, k, nr, j, status, _ = run_pdlp(eng, tol=tol, verbose=False, primal_update=True, seed=3, precondition=True)
    print(f"37x23 lowrank, Ruiz + Pock-Chambolle: k={k} n={nr} j={j} objective {obj:.12g} (opt {qp.opt:.12g})")
    assert status == "Solved", (status, k)
    assert abs(obj - qp.opt) <= bound_of(tol, qp.opt), (obj, qp.opt)
    xu = x.numpy() * dc
    assert abs(model_of_general_qp(qp).objective(xu) - obj) <= 1e-9 * (1 + abs(obj))


def test_the_step_changes_after_a_restart_that_changes_omega_and_only_then():
    qp = make_general_qp(37, 23, 1, None, "lowrank")
    mo = model_of_general_qp(qp)
    eng = GeneralQuadEngine(mo)
    tr = dict(kkt=[], omega=[], restarts=[])
    sigma = float(np.linalg.norm(mo.A, 2))
    L = float(np.linalg.norm(mo.Q, 2))
    assert abs(estimate_quad_norm(eng, seed=3) - L) <= 1e-6 * L
    out = run_pdlp(eng, tol=1e-8, verbose=False, primal_update=True, sigma=sigma, quad_norm=L, trace=tr)
    assert out[5] == "Solved" and len(tr["restarts"]) >= 5
    # the first step at the start weight, then one step per restart whose primal weight differs from the one before
    omegas = [eng.steps[0][1]] + tr["omega"]
    changed = [i for i in range(1, len(omegas)) if omegas[i] != omegas[i - 1]]
    assert len(changed) >= 4
    assert len(eng.steps) == 1 + len(changed) == len(tr["eta"])
    assert [s[1] for s in eng.steps[1:]] == [omegas[i] for i in changed]
    assert len(eng.omegas) == len(tr["omega"]) - len(changed)              # (a restart that leaves omega alone sets it alone)
    at = [r[1] for r in tr["restarts"]]                                     # (iterations since the previous restart)
    restart_iters = set(np.cumsum(at).tolist())
    assert eng.steps[0][2] == 0 and all(s[2] in restart_iters for s in eng.steps[1:])
    for (eta, omega, _), traced in zip(eng.steps, tr["eta"]):
        assert eta == traced == float(qp_eta(sigma, L, omega, np.float64))
    assert all(a[0] != b[0] for a, b in zip(eng.steps, eng.steps[1:]))
    # without the primal weight update nothing changes omega: the step is set once
    eng = GeneralQuadEngine(mo)
    run_pdlp(eng, tol=1e-4, verbose=False, primal_update=False, sigma=sigma, quad_norm=L)
    assert len(eng.steps) == 1 and not eng.omegas
    # an LP engine's driver never touches the step after the start, as before
    lin = QuadModelEngine(model_of_qp(make_qp(37, 23, 1)))
    calls = []
    lin.set_step = lambda *a, _f=lin.set_step: (calls.append(a), _f(*a))[1]
    run_pdlp(lin, tol=1e-4, verbose=False, primal_update=True, sigma=sigma)
    assert len(calls) == 1


def test_a_diagonal_matrix_and_quad_diag_reach_the_same_optimum():
    import scipy.sparse as sp
    qp = make_qp(40, 60, 1)
    tol = 1e-8
    sigma = float(np.linalg.norm(qp.A.toarray(), 2))
    by_diag = run_pdlp(QuadModelEngine(model_of_qp(qp)), tol=tol, verbose=False, primal_update=True, sigma=sigma)
    mo = GeneralQuadModel(qp.A, qp.m_ineq, qp.c, qp.q, qp.l, qp.u, sp.diags(qp.d).tocsr())
    by_matrix = run_pdlp(GeneralQuadEngine(mo), tol=tol, verbose=False, primal_update=True, sigma=sigma, seed=3)
    assert by_diag[5] == by_matrix[5] == "Solved"
    for obj in (by_diag[1], by_matrix[1]):
        assert abs(obj - qp.opt) <= bound_of(tol, qp.opt), (obj, qp.opt)
    assert abs(by_diag[1] - by_matrix[1]) <= 2 * bound_of(tol, qp.opt)
    print(f"quad_diag k={by_diag[2]}, the same term as quad_matrix k={by_matrix[2]}")
