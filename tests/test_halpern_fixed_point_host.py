"""The fixed-point-error restart rule of the Halpern mode on the host (halpern_restart="fixed_point"): rules.fixed_point_error and
rules.fixed_point_restart_decision against hand-computed cases, the refusals of the entry functions, and PdhgDriver over a numpy
engine against the method stated straight down -- call sequence, counters, restart list (no GPU)."""
import numpy as np
import pytest
import torch

from tests.halpern_fp_model import FixedPointModelEngine, expected_calls, fixed_point_driver_model
from tests.ranged_model import RangedModel, feasible_ranged_lp
from torchpdlp_amd import _native as N
from torchpdlp_amd import rules
from torchpdlp_amd.solver import PdhgDriver, pdlp_algorithm, run_pdlp

TYPES = [np.float32, np.float64]
INF = np.inf


# ---------------------------------------------------------------------------------------------------
# rules.fixed_point_error
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES, ids=["f32", "f64"])
def test_fixed_point_error_by_hand(t):
    # eta = 1/2, omega = 2: omega/eta = 4, 1/(eta omega) = 1; r^2 = 4 * 3 - 2 * 1.5 + 7 = 16 (every number exact in both types)
    r = rules.fixed_point_error(t(3), t(1.5), t(7), t(0.5), t(2))
    assert type(r) is np.float64 and r == 4.0
    # eta = 1/4, omega = 1/2: omega/eta = 2, 1/(eta omega) = 8; r^2 = 2 * 2 + 2 * 0.5 + 8 * 0.5 = 9 (a negative cross term adds)
    assert rules.fixed_point_error(t(2), t(-0.5), t(0.5), t(0.25), t(0.5)) == 3.0
    # formed in double whatever the type of eta and omega: eta = float32(0.1) is used as the double it is
    e = np.float32(0.1)
    want = np.sqrt(np.float64(3) / np.float64(e) * 2.0 - 2 * 0.25 + 5.0 / (np.float64(e) * np.float64(3)))
    assert rules.fixed_point_error(2.0, 0.25, 5.0, e, np.float32(3)) == want
    # the point is a fixed point
    assert rules.fixed_point_error(0.0, 0.0, 0.0, t(0.5), t(2)) == 0.0


@pytest.mark.parametrize("t", TYPES, ids=["f32", "f64"])
def test_fixed_point_error_clips_a_negative_square(t):
    # 4 * 1 - 2 * 4 + 1 = -3: rounding can do this when the three terms cancel; the residual is 0, not nan
    with np.errstate(invalid="raise"):
        r = rules.fixed_point_error(t(1), t(4), t(1), t(0.5), t(2))
    assert r == 0.0 and not np.isnan(r)
    # arrays, element by element
    r = rules.fixed_point_error(np.array([3.0, 1.0], t), np.array([1.5, 4.0], t), np.array([7.0, 1.0], t), t(0.5), t(2))
    assert r.tolist() == [4.0, 0.0]


# ---------------------------------------------------------------------------------------------------
# rules.fixed_point_restart_decision
# ---------------------------------------------------------------------------------------------------
def decide(t, r, r_prev, r0, tt, k, **kw):
    d = rules.fixed_point_restart_decision(r, r_prev, r0, tt, k, t=t, **kw)
    assert set(d) == {"crit", "use_avg", "capped", "action"}                  # (restart_decision's dict)
    assert bool(d["use_avg"]) == (int(d["crit"]) >= 0) and int(d["action"]) in (0, 1, 2)
    assert (int(d["action"]) == 2) == (int(d["crit"]) >= 0)
    return int(d["crit"])


@pytest.mark.parametrize("t", TYPES, ids=["f32", "f64"])
def test_each_criterion_alone(t):
    # r0 = 8 (0.2 r0 = 1.6, 0.8 r0 = 6.4 up to the rounding of the constants); tt = 40 of k = 400: 40 < 144, no artificial restart
    assert decide(t, 1.5, 7.0, 8.0, 40, 400) == 0                             # sufficient: 1.5 <= 1.6 (and no growth: not necessary)
    assert decide(t, 6.0, 5.0, 8.0, 40, 400) == 1                             # necessary: 6 <= 6.4 and 6 > 5
    assert decide(t, 6.0, 6.5, 8.0, 40, 400) == -1                            # ... but not while the residual still falls
    assert decide(t, 7.0, 5.0, 8.0, 40, 400) == -1                            # ... nor above 0.8 r0, growth or not
    assert decide(t, 7.0, 7.5, 8.0, 160, 400) == 2                            # artificial: 160 >= 0.36 * 400 = 144
    assert decide(t, 7.0, 7.5, 8.0, 143, 400) == -1
    assert decide(t, 7.0, 7.5, 8.0, 144, 400) == 2                            # (>=)
    # the thresholds themselves, with the constants rounded to the working precision as restart_decision rounds them
    s, nq = t(rules.BETA[0]) * t(8), t(rules.BETA[1]) * t(8)
    assert decide(t, s, INF, 8.0, 40, 400) == 0 and decide(t, np.nextafter(s, t(INF)), INF, 8.0, 40, 400) == -1
    assert decide(t, nq, 1.0, 8.0, 40, 400) == 1 and decide(t, np.nextafter(nq, t(INF)), 1.0, 8.0, 40, 400) == -1
    assert decide(t, 6.0, 6.0, 8.0, 40, 400) == -1                            # r > r_prev is strict


@pytest.mark.parametrize("t", TYPES, ids=["f32", "f64"])
def test_priority_first_check_zero_r0_and_dead(t):
    # all three hold: sufficient wins; necessary and artificial: necessary wins
    assert decide(t, 1.0, 0.5, 8.0, 400, 400) == 0
    assert decide(t, 6.0, 5.0, 8.0, 400, 400) == 1
    # the first check of a period: r_prev = inf, so the necessary criterion cannot fire whatever r is
    assert decide(t, 6.0, INF, 8.0, 40, 400) == -1
    assert decide(t, 1.5, INF, 8.0, 40, 400) == 0
    assert decide(t, 6.0, INF, 8.0, 40, 40) == 2                              # (the first check of a run: 40 >= 14.4)
    # r0 = 0 (the restart point was a fixed point): only r = 0 is "sufficient"; anything else waits for the artificial restart
    assert decide(t, 0.0, INF, 0.0, 40, 400) == 0
    assert decide(t, 1e-30, INF, 0.0, 40, 400) == -1 and decide(t, 1e-30, 0.0, 0.0, 40, 400) == -1
    assert decide(t, 1e-30, 0.0, 0.0, 200, 400) == 2
    # arrays, and LPs that are not live
    d = rules.fixed_point_restart_decision(np.array([1.5, 6.0, 7.0, 1.5]), np.array([7.0, 5.0, 7.5, 7.0]), np.full(4, 8.0),
                                           np.array([40, 40, 160, 40]), np.full(4, 400), live=np.array([True, True, True, False]), t=t)
    assert d["crit"].tolist() == [0, 1, 2, -1] and d["use_avg"].tolist() == [True, True, True, False]
    assert d["action"].tolist() == [2, 2, 2, 0]
    # the KKT-pass cap, as in restart_decision: no restart and j at the cap
    d = rules.fixed_point_restart_decision(7.0, 7.5, 8.0, 40, 400, j=100, max_kkt=100, t=t)
    assert int(d["crit"]) == -1 and bool(d["capped"]) and int(d["action"]) == 1


def test_restart_decision_is_untouched():
    """the averaged method's rule still takes the KKT errors: sufficient at the average, by hand"""
    d = rules.restart_decision(2.0, 1.0, 3.0, 8.0, 40, 400, 0)
    assert int(d["crit"]) == 0 and bool(d["use_avg"]) and int(d["action"]) == 2


# ---------------------------------------------------------------------------------------------------
# refusals: before any device work, before an engine is used
# ---------------------------------------------------------------------------------------------------
class Untouchable:
    comm, mixed = None, False

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} was used")


def test_refusals_raise_before_any_device_work():
    import torchpdlp_amd as tp
    K, v = torch.eye(3), torch.zeros(3)
    for kw, match in ((dict(halpern_restart="fixed_point"), "needs halpern=True"), (dict(halpern_restart="fixed_point", halpern=False), "needs halpern=True"),
                      (dict(halpern=True, halpern_restart="residual"), "unknown halpern_restart"),
                      (dict(halpern_restart="KKT"), "unknown halpern_restart"), (dict(halpern=True, halpern_restart=None), "unknown halpern_restart")):
        with pytest.raises(ValueError, match=match):
            pdlp_algorithm(K, 1, v, v, v, v + 1, "cpu", verbose=False, **kw)
        with pytest.raises(ValueError, match=match):
            tp.solve_lp((v, K, v, 1, v, v + 1), device="cpu", **kw)
        with pytest.raises(ValueError, match=match):
            run_pdlp(Untouchable(), verbose=False, sigma=1.0, **kw)
        with pytest.raises(ValueError, match=match):
            PdhgDriver(Untouchable(), **kw)
    # the refusals of the Halpern mode itself hold under the new rule too
    with pytest.raises(ValueError, match="halpern"):
        run_pdlp(Untouchable(), verbose=False, halpern=True, halpern_restart="fixed_point", adaptive=True, sigma=1.0)
    with pytest.raises(ValueError, match="halpern"):
        tp.solve_lp((v, K, v, 1, v, v + 1), device="cpu", halpern=True, halpern_restart="fixed_point", precision="mixed")


def test_batch_solve_does_not_take_the_keyword():
    import torchpdlp_amd as tp
    K, v = torch.eye(3), torch.zeros(3, 2)
    with pytest.raises(TypeError):
        tp.solve_lp_batch((v, K, v, 1, v, v + 1), device="cpu", halpern=True, halpern_restart="fixed_point")


def test_library_and_cli_have_the_call():
    lib = N.load()
    assert "pdlp_halpern_fixed_point" in N.SIGNATURES and N.ABI_VERSION == 18 == lib.pdlp_abi_version()
    assert lib.pdlp_halpern_fixed_point(None) == -1                           # PDLP_ERR_INVALID
    from torchpdlp_amd.__main__ import parse_args
    assert parse_args([]).halpern_restart == "kkt"
    assert parse_args(["--halpern", "--halpern_restart", "fixed_point"]).halpern_restart == "fixed_point"
    with pytest.raises(SystemExit):
        parse_args(["--halpern_restart", "other"])


# ---------------------------------------------------------------------------------------------------
# the driver over a numpy engine
# ---------------------------------------------------------------------------------------------------
def ranged_model(seed=2, m=40, n=60):
    A, m_ineq, c, q, l, u, qu = feasible_ranged_lp(m, n, 4, seed)
    return RangedModel(A, m_ineq, c, q, l, u, qu)


@pytest.mark.parametrize("pw", [False, True], ids=["nopw", "pw"])
@pytest.mark.parametrize("period", [40, 7])
def test_driver_runs_the_method_as_stated(period, pw):
    """run_pdlp(halpern=True, halpern_restart="fixed_point") over the numpy engine and the straight-line statement take the same
    path with the same arithmetic: counters, restart list and x are equal, exactly; the engine saw halpern_iterate(1),
    halpern_fixed_point, halpern_iterate(period - 1), halpern_fixed_point, ... with no KKT pass at a check; j = iterations + one
    per evaluation (r0 of every period and every check) + two per restart."""
    mo = ranged_model()
    sigma = float(np.linalg.norm(mo.A, 2))
    eng, trace = FixedPointModelEngine(mo), dict(kkt=[], omega=[], restarts=[])
    x, obj, k, n, j, status, _ = run_pdlp(eng, tol=1e-6, verbose=False, primal_update=pw, sigma=sigma, trace=trace, halpern=True,
                                          halpern_restart="fixed_point", restart_period=period)
    ref = fixed_point_driver_model(mo, sigma, 1e-6, pw, period)
    assert status == "Solved" == ref["status"]
    assert (k, n, j) == (ref["k"], ref["n"], ref["j"])
    assert trace["restarts"] == ref["restarts"] and n >= 3
    assert np.array_equal(x.numpy(), ref["x"])
    checks = k // period
    assert k % period == 0 and j == k + n + checks + 2 * n                    # (one r0 per restart period: the run ends at a restart)
    assert eng.calls == expected_calls(ref["restarts"], checks, period, pw)
    # what the trace receives at a check: [inf, r, r_prev], r_prev = inf at the first check of a period; then KKT_first per restart
    flat, at, tt = trace["kkt"], 0, 0
    left = list(ref["restarts"])
    for _ in range(checks):
        cur, r, r_prev = flat[at:at + 3]
        at, tt = at + 3, tt + period
        assert np.isinf(cur) and np.isfinite(r) and (np.isinf(r_prev) == (tt == period))
        if left and left[0][1] == tt:
            left.pop(0)
            at, tt = at + 1, 0
    assert at == len(flat)
    assert all(c in (0, 1, 2) and u == 1 for c, _, u in trace["restarts"])
    assert len(trace["omega"]) == (n if pw else 0)


def test_keyword_kkt_is_the_default_path():
    """halpern=True with the keyword omitted and with "kkt": the same calls, counters and x (the candidate's KKT error decides)"""
    mo = ranged_model()
    sigma = float(np.linalg.norm(mo.A, 2))
    runs = []
    for kw in ({}, dict(halpern_restart="kkt")):
        eng, trace = FixedPointModelEngine(mo), dict(kkt=[], omega=[], restarts=[])
        out = run_pdlp(eng, tol=1e-6, verbose=False, primal_update=True, sigma=sigma, trace=trace, halpern=True, **kw)
        assert ("halpern_fixed_point",) not in eng.calls and ("kkt", N.AVG) in eng.calls
        runs.append((out[0].numpy().tolist(), out[1:6], trace, eng.calls))
    assert runs[0] == runs[1]
