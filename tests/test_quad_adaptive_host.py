"""The adaptive step of the sparse quadratic objective on the host (no GPU): the refusals of ``quad_step`` before device work, the
default against today's trace on the numpy engine, the table of DESIGN.md 4.5.1 on the float64 model of
tests/qp_adaptive_model.py, a ``Q`` without stored entries against the LP's rule, and the library's entry point."""
import numpy as np
import pytest
import torch

import torchpdlp_amd as tp
from tests.qp_adaptive_model import AdaptiveQuadEngine, AdaptiveQuadModel, adaptive_model_of
from tests.qp_model import GeneralQuadEngine, make_general_qp, model_of_general_qp
from tests.ranged_model import RangedModel
from tests.test_quad_matrix_host import bound_of
from torchpdlp_amd import _native as N
from torchpdlp_amd.compose import QMAT_REFUSED, QUAD_STEPS, check_quad_step
from torchpdlp_amd.rules import qp_eta
from torchpdlp_amd.solver import PdhgDriver, pdlp_algorithm, run_pdlp

K3 = torch.eye(3)
V3 = torch.zeros(3)
Q3 = torch.tensor([[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 0.0]])
LP3 = (V3, K3, V3, 2, V3, V3 + 1)


# ---------------------------------------------------------------------------------------------------
# 1. the keyword's refusals, all before device work
# ---------------------------------------------------------------------------------------------------
def test_quad_step_values():
    assert QUAD_STEPS == ("fixed", "adaptive")
    assert check_quad_step("fixed", False) == check_quad_step("fixed", True) == "fixed"
    assert check_quad_step("adaptive", True) == "adaptive"
    for bad in ("Adaptive", "", None, True, "malitsky"):
        with pytest.raises(ValueError, match="quad_step"):
            check_quad_step(bad, True)
    with pytest.raises(ValueError, match="needs quad_matrix"):
        check_quad_step("adaptive", False)


def test_unknown_value_and_missing_matrix_raise_before_any_device_work():
    for kw in (dict(quad_step="newton", quad_matrix=Q3), dict(quad_step="newton"), dict(quad_step="adaptive")):
        with pytest.raises(ValueError, match="quad_step"):
            tp.solve_lp(LP3, device="cpu", **kw)
        with pytest.raises(ValueError, match="quad_step"):
            pdlp_algorithm(K3, 2, V3, V3, V3, V3 + 1, "cpu", verbose=False, **kw)
    # ... and the accepted values reach the device: with device="cpu" that is the first failure
    for step in QUAD_STEPS:
        with pytest.raises(Exception) as e:
            tp.solve_lp(LP3, device="cpu", quad_matrix=Q3, quad_step=step)
        assert not isinstance(e.value, ValueError)


REFUSALS = [dict(adaptive=True), dict(halpern=True), dict(adaptive=True, adaptive_retry=True), dict(infeasibility_detect=True),
            dict(precision="mixed"), dict(comm=True), dict(direct_exchange=True), dict(fishnet=True)]


@pytest.mark.parametrize("kw", REFUSALS, ids=lambda kw: "+".join(kw))
def test_what_quad_matrix_refuses_stays_refused_with_the_text_unchanged(kw):
    names = dict(adaptive="adaptive_stepsize")
    with pytest.raises(ValueError) as e:
        tp.solve_lp(LP3, device="cpu", quad_matrix=Q3, quad_step="adaptive", **{names.get(k, k): v for k, v in kw.items()})
    assert str(e.value) == QMAT_REFUSED
    if not ({"fishnet", "direct_exchange"} & set(kw)):                    # (these two are solve_lp's flags)
        with pytest.raises(ValueError) as e:
            pdlp_algorithm(K3, 2, V3, V3, V3, V3 + 1, "cpu", verbose=False, quad_matrix=Q3, quad_step="adaptive", **kw)
        assert str(e.value) == QMAT_REFUSED


class _Untouched:
    """an engine the driver must refuse before it uses it"""
    comm, mixed, delta, q_upper, quad_diag, m_ineq = None, False, False, None, None, 1
    dtype = torch.float32

    def __init__(self, quad_matrix):
        self.quad_matrix = quad_matrix

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} was used")


def test_driver_refuses_before_the_engine_is_used():
    with pytest.raises(ValueError, match="needs quad_matrix"):
        run_pdlp(_Untouched(None), verbose=False, sigma=1.0, quad_step="adaptive")
    with pytest.raises(ValueError, match="unknown quad_step"):
        run_pdlp(_Untouched(Q3), verbose=False, sigma=1.0, quad_step="both")
    for kw in (dict(adaptive=True), dict(halpern=True), dict(infeasibility_detect=True), dict(adaptive=True, adaptive_retry=True)):
        with pytest.raises(ValueError) as e:
            run_pdlp(_Untouched(Q3), verbose=False, sigma=1.0, quad_step="adaptive", **kw)
        assert str(e.value) == QMAT_REFUSED
    with pytest.raises(ValueError, match="needs quad_matrix"):
        PdhgDriver(_Untouched(None), quad_step="adaptive")


def test_solve_lp_batch_has_no_such_keyword():
    with pytest.raises(TypeError):
        tp.solve_lp_batch(LP3, device="cpu", quad_step="adaptive")


# ---------------------------------------------------------------------------------------------------
# 2. the default is today's solve
# ---------------------------------------------------------------------------------------------------
def test_the_default_is_the_fixed_step_call_for_call():
    """without the keyword, and with "fixed", the driver makes the calls it made before the keyword existed: ``iterate(n, False)``
    segments, ``flush_average(False)``, the step set anew after every restart that changes omega -- the record of
    tests/test_quad_matrix_host.py's trace test -- and never ``objective_iterate``"""
    qp = make_general_qp(37, 23, 1, None, "lowrank")
    runs = []
    for kw in ({}, dict(quad_step="fixed")):
        eng = GeneralQuadEngine(model_of_general_qp(qp))
        calls = []
        eng.iterate = lambda n, adaptive, _f=eng.iterate: (calls.append(("iterate", int(n), bool(adaptive))), _f(n, adaptive))[1]
        eng.flush_average = lambda adaptive=True: calls.append(("flush", bool(adaptive)))
        eng.objective_iterate = lambda n: (_ for _ in ()).throw(AssertionError("objective_iterate under the fixed step"))
        tr = dict(kkt=[], omega=[], restarts=[])
        out = run_pdlp(eng, tol=1e-8, verbose=False, primal_update=True, seed=3, trace=tr, **kw)
        runs.append((out[1:6], eng.steps, eng.omegas, tr, calls, out[0].numpy()))
    a, b = runs
    assert a[:5] == b[:5] and np.array_equal(a[5], b[5])
    assert a[0][1:] == (600, 10, a[0][3], "Solved")                         # (the fixed-step row of the table below)
    assert all(c[2] is False for c in a[4] if c[0] == "iterate") and all(c[1] is False for c in a[4] if c[0] == "flush")
    omegas = [a[1][0][1]] + a[3]["omega"]
    changed = [i for i in range(1, len(omegas)) if omegas[i] != omegas[i - 1]]
    assert len(a[1]) == 1 + len(changed) >= 5 and len(a[2]) == len(a[3]["omega"]) - len(changed)


def test_the_adaptive_driver_keeps_eta_and_sets_omega_alone():
    qp = make_general_qp(37, 23, 1, None, "lowrank")
    mo = adaptive_model_of(qp)
    eng = AdaptiveQuadEngine(mo)
    calls = []
    eng.flush_average = lambda adaptive=True: calls.append(bool(adaptive))
    eng.iterate = lambda *a: (_ for _ in ()).throw(AssertionError("iterate under quad_step='adaptive'"))
    tr = dict(kkt=[], omega=[], restarts=[])
    sigma, L = float(np.linalg.norm(mo.A, 2)), float(np.linalg.norm(mo.Q, 2))
    x, obj, k, nr, j, status, _ = run_pdlp(eng, tol=1e-8, verbose=False, primal_update=True, sigma=sigma, quad_norm=L, trace=tr,
                                           quad_step="adaptive")
    assert status == "Solved" and nr >= 5
    # the start step is qp_eta at the start weight; afterwards the driver never sets a step, only the primal weight
    assert len(eng.steps) == 1 and eng.steps[0][0] == float(qp_eta(sigma, L, eng.steps[0][1], np.float64)) and eng.steps[0][2] == 0
    assert tr["eta"] == [eng.steps[0][0]]
    assert len(eng.omegas) == len(tr["omega"]) == nr and len(set(eng.omegas)) >= 4
    assert calls and all(calls)                                              # (the average is flushed as for an adaptive LP)
    # KKT-pass accounting of an adaptive LP solve: one per iteration, three per check, two per restart
    checks = k // 40
    assert k % 40 == 0 and j == k + 3 * checks + 2 * nr


# ---------------------------------------------------------------------------------------------------
# 3. the table of DESIGN.md 4.5.1 on the model
# ---------------------------------------------------------------------------------------------------
# (m, n, per_row, kind, tol, seed): (fixed iterations, restarts), (adaptive iterations, restarts), (accepted, rejected)
TABLE = {
    (37, 23, None, "lowrank", 1e-8, 1): ((600, 10), (280, 7), (280, 0)),
    (37, 23, None, "lowrank", 1e-8, 2): ((800, 9), (440, 8), (433, 7)),
    (37, 23, None, "lowrank", 1e-4, 1): ((280, 5), (160, 4), (160, 0)),
    (37, 23, None, "lowrank", 1e-4, 2): ((240, 4), (200, 4), (198, 2)),
    (600, 520, 8, "sparse", 1e-4, 1): ((640, 6), (400, 5), (394, 6)),
    (600, 520, 8, "sparse", 1e-4, 2): ((720, 6), (280, 4), (267, 13)),
    (300, 2600, 6, "arrow", 1e-4, 1): ((200, 4), (120, 3), (115, 5)),
    (300, 2600, 6, "arrow", 1e-4, 2): ((320, 5), (200, 4), (185, 15)),
}
# the objective of the 37 x 23, seed 1, 1e-8 adaptive run is 3.3e-8 relative from the optimum ; bound_of(1e-8, opt)
# = 2e-8 (1 + 2 |opt|) with |opt| = 10.67 is 3.8e-8 (1 + |opt|): inside


@pytest.mark.parametrize("row", list(TABLE), ids=lambda r: f"{r[0]}x{r[1]}_{r[3]}_{r[4]:g}_seed{r[5]}")
def test_the_table_of_the_design_document(row):
    m, n, per_row, kind, tol, seed = row
    fixed, adaptive, trials = TABLE[row]
    qp = make_general_qp(m, n, seed, per_row, kind)
    f = run_pdlp(GeneralQuadEngine(adaptive_model_of(qp)), tol=tol, verbose=False, primal_update=True, seed=3)
    eng = AdaptiveQuadEngine(adaptive_model_of(qp))
    x, obj, k, nr, j, status, _ = run_pdlp(eng, tol=tol, verbose=False, primal_update=True, seed=3, quad_step="adaptive")
    rel = abs(obj - qp.opt) / (1 + abs(qp.opt))
    print(f"{row}: fixed k={f[2]} n={f[3]}; adaptive k={k} n={nr} j={j} accepted/rejected {eng.accepted}/{eng.rejected} "
          f"objective {obj:.12g} (opt {qp.opt:.12g}, relative {rel:.3g})")
    assert f[5] == status == "Solved"
    assert (f[2], f[3]) == fixed and (k, nr) == adaptive and (eng.accepted, eng.rejected) == trials
    assert k < f[2]
    assert rel <= (1.1e-4 if tol == 1e-4 else 3.3e-8)
    assert abs(obj - qp.opt) <= bound_of(tol, qp.opt), (obj, qp.opt)
    xv = x.numpy()
    assert (xv >= qp.l).all() and (xv <= qp.u).all()


def test_the_seed_1_rows_do_not_depend_on_the_weight_of_an_accepted_trial():
    """the library weighs an accepted trial with the step size it used, the table's model with the one the rule left behind: the
    counts the GPU solves are compared with are the same under both"""
    for (m, n, per_row, kind, tol, seed), (_, adaptive, _) in TABLE.items():
        if seed != 1:
            continue
        qp = make_general_qp(m, n, seed, per_row, kind)
        out = run_pdlp(AdaptiveQuadEngine(adaptive_model_of(qp), weights="used"), tol=tol, verbose=False, primal_update=True, seed=3,
                       quad_step="adaptive")
        assert (out[2], out[3], out[5]) == adaptive + ("Solved",)


# ---------------------------------------------------------------------------------------------------
# 4. the rule itself
# ---------------------------------------------------------------------------------------------------
def _point(qp, seed=3):
    rng = np.random.default_rng(seed)
    lo, hi = np.where(np.isinf(qp.l), -3, qp.l), np.where(np.isinf(qp.u), 3, qp.u)
    y = rng.standard_normal(qp.m)
    y[:qp.m_ineq] = np.abs(y[:qp.m_ineq])
    return np.clip(rng.standard_normal(qp.n), lo, hi), y


def test_a_matrix_without_entries_follows_the_rule_of_the_lp_exactly():
    qp = make_general_qp(37, 23, 1, None, "lowrank")
    zero = AdaptiveQuadModel(qp.A, qp.m_ineq, qp.c, qp.q, qp.l, qp.u, None, qp.d)
    lin = RangedModel(qp.A, qp.m_ineq, qp.c, qp.q, qp.l, qp.u)
    assert not zero.Q.any() and not zero.d.any()
    x, y = _point(qp)
    xl, yl, eta, el = x, y, 0.07, 0.07
    for k in range(1, 13):
        x, y, eta = zero.adaptive_step(x, y, eta, 0.8, k)
        xl, yl, el = lin.adaptive_step(xl, yl, el, 0.8, k)
        assert np.array_equal(x, xl) and np.array_equal(y, yl) and eta == el
    assert eta != 0.07


def test_the_curvature_is_the_descent_lemma_term_and_only_tightens():
    qp = make_general_qp(600, 520, 1, 8, "sparse")
    mo = adaptive_model_of(qp)
    x, y = _point(qp)
    for eta in (0.02, 0.2, 2.0):
        full, lp = mo.rule(x, y, eta, 0.8, 1), mo.rule(x, y, eta, 0.8, 1, curvature=False)
        dx = full.x - x
        assert full.curv > 0 and abs(full.curv - dx @ (full.g_new - full.g)) <= 1e-12 * full.curv      # (what the epilogue sums)
        assert np.array_equal(full.x, lp.x) and full.eta_bar < lp.eta_bar
        assert full.eta_bar == (0.8 * full.nx2 + full.ny2 / 0.8) / (abs(full.den) + full.curv)
        assert full.weight == (eta if full.accepted else full.eta_next)
    # K = 0: the bound is tau <= 1 / lambda along the direction moved
    free = AdaptiveQuadModel(np.zeros((1, 3)), 0, [1.0, -2.0, 0.5], [0.0], [-np.inf] * 3, [np.inf] * 3, np.diag([4.0, 1.0, 0.25]))
    r = free.rule(np.zeros(3), np.zeros(1), 0.5, 1.0, 1)
    dx = r.x
    assert r.den == 0 and abs(r.eta_bar - (dx @ dx) / (dx @ (free.Q @ dx))) <= 1e-15


# ---------------------------------------------------------------------------------------------------
# 5. the library
# ---------------------------------------------------------------------------------------------------
def test_library_entry_point():
    lib = N.load()
    assert "pdlp_objective_iterate" in N.SIGNATURES
    assert N.ABI_VERSION == 18 == lib.pdlp_abi_version()
    assert lib.pdlp_objective_iterate(None, 1) == -1
    assert N.S_CURV == 13 < N.NSCAL == 16
