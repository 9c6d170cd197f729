"""The diagonal quadratic objective on the host (no GPU): the validation of ``quad_diag`` and every refusal before device work, the
scaling rule ``d_s = d D_col^2`` with the invariance of ``1/2 x'Dx`` and of the un-scaled KKT numbers, and ``run_pdlp`` over a float64
numpy engine that implements the arithmetic (tests/quad_model.py) on problems with a constructed optimum."""
import numpy as np
import pytest
import torch

import torchpdlp_amd as tp
from tests.quad_model import QuadModel, QuadModelEngine, make_qp, model_of_qp
from torchpdlp_amd import _native as N
from torchpdlp_amd.quad import REFUSED, check_quad_diag
from torchpdlp_amd.solver import pdlp_algorithm, run_pdlp

INF = float("inf")
K3 = torch.eye(3)
V3 = torch.zeros(3)
D3 = torch.tensor([1.0, 0.0, 2.0])
BAD = {"length": [1.0, 2.0], "negative": [1.0, -0.5, 0.0], "nan": [float("nan"), 0.0, 0.0], "inf": [INF, 0.0, 0.0],
       "minus_inf": [-INF, 0.0, 0.0], "matrix": [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], "column_wrong_length": [[1.0], [2.0]],
       "scalar": 1.0}


# ---------------------------------------------------------------------------------------------------
# 1. validation and refusals, all before device work
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BAD))
def test_malformed_quad_diag_raises_before_any_device_work(name):
    d = torch.tensor(BAD[name])
    with pytest.raises(ValueError, match="quad_diag"):
        check_quad_diag(d, 3)
    with pytest.raises(ValueError, match="quad_diag"):
        pdlp_algorithm(K3, 2, V3, V3, V3, V3 + 1, "cpu", verbose=False, quad_diag=d)
    with pytest.raises(ValueError, match="quad_diag"):
        tp.solve_lp((V3, K3, V3, 2, V3, V3 + 1), device="cpu", quad_diag=d)


def test_well_formed_quad_diag_passes_the_check():
    for ok in (D3, D3.view(-1, 1), D3.double(), torch.zeros(3), D3.numpy(), [0.0, 1.0, 2.0], torch.tensor([1, 0, 2])):
        out = check_quad_diag(ok, 3)
        assert out.shape == (3,)
    assert check_quad_diag(None, 3) is None
    # ... and then reaches the device: on a machine without one, or with device="cpu", that is the first failure
    with pytest.raises(Exception) as e:
        tp.solve_lp((V3, K3, V3, 2, V3, V3 + 1), device="cpu", quad_diag=D3)
    assert not isinstance(e.value, ValueError)


REFUSALS = [dict(precision="mixed"), dict(comm=True), dict(infeasibility_detect=True), dict(adaptive=True, adaptive_retry=True),
            dict(fishnet=True)]


@pytest.mark.parametrize("kw", REFUSALS, ids=lambda kw: "+".join(kw))
def test_refused_combinations_raise_before_any_device_work(kw):
    names = dict(adaptive="adaptive_stepsize")
    with pytest.raises(ValueError, match="quad_diag") as e:
        tp.solve_lp((V3, K3, V3, 2, V3, V3 + 1), device="cpu", quad_diag=D3, **{names.get(k, k): v for k, v in kw.items()})
    assert str(e.value) == REFUSED
    if "fishnet" not in kw:                            # (fishnet is solve_lp's flag)
        with pytest.raises(ValueError, match="quad_diag"):
            pdlp_algorithm(K3, 2, V3, V3, V3, V3 + 1, "cpu", verbose=False, quad_diag=D3, **kw)
    # together with q_upper, which refuses the same flags: still a ValueError before device work
    with pytest.raises(ValueError):
        tp.solve_lp((V3, K3, V3, 2, V3, V3 + 1), device="cpu", quad_diag=D3, q_upper=torch.tensor([1.0, INF, INF]),
                    **{names.get(k, k): v for k, v in kw.items()})


def test_direct_exchange_is_refused_and_a_path_is_checked_before_it_is_read():
    with pytest.raises(ValueError, match="quad_diag") as e:
        tp.solve_lp((V3, K3, V3, 2, V3, V3 + 1), device="cpu", quad_diag=D3, direct_exchange=True)
    assert "direct_exchange" in str(e.value) == REFUSED
    # an MPS path: a malformed vector is a ValueError before the file is even opened (its length is compared once n is known)
    for bad in ("negative", "nan", "inf", "matrix", "scalar"):
        with pytest.raises(ValueError, match="quad_diag"):
            tp.solve_lp("no/such/file.mps", device="cpu", quad_diag=torch.tensor(BAD[bad]))
    with pytest.raises(Exception) as e:
        tp.solve_lp("no/such/file.mps", device="cpu", quad_diag=D3)
    assert not isinstance(e.value, ValueError)


def test_the_batch_has_no_keyword():
    with pytest.raises(TypeError, match="quad_diag"):
        tp.solve_lp_batch((V3, K3, V3, 2, V3, V3 + 1), device="cpu", quad_diag=D3)


def test_driver_refuses_too():
    """run_pdlp / PdhgDriver over an engine that has quad_diag: the same refusals, before the engine is used"""
    class Engine:
        comm, mixed, delta, q_upper, quad_diag, m_ineq = None, False, False, None, torch.tensor([1.0]), 1
        dtype = torch.float32

        def __getattr__(self, name):
            raise AssertionError(f"engine.{name} was used")
    for kw in (dict(infeasibility_detect=True), dict(adaptive=True, adaptive_retry=True)):
        with pytest.raises(ValueError, match="quad_diag"):
            run_pdlp(Engine(), verbose=False, sigma=1.0, **kw)

    class Mixed(Engine):
        mixed = True
    with pytest.raises(ValueError, match="quad_diag"):
        run_pdlp(Mixed(), verbose=False, sigma=1.0)


def test_library_entry_point():
    lib = N.load()
    assert "pdlp_set_objective_diag" in N.SIGNATURES and N.ABI_VERSION == 18 == lib.pdlp_abi_version()
    assert lib.pdlp_set_objective_diag(None, None) == -1


# ---------------------------------------------------------------------------------------------------
# 2. the scaling rule
# ---------------------------------------------------------------------------------------------------
def test_scaling_returns_d_times_d_col_squared():
    s = tp.Scaling(torch.tensor([2.0, 0.5]), torch.tensor([4.0, 0.25, 2.0]))
    c, q, l, u = torch.ones(2), torch.tensor([1.0, -2.0, 3.0]), torch.zeros(2), torch.ones(2)
    d, qu = torch.tensor([3.0, 8.0]), torch.tensor([2.0, INF, 3.0])
    four, five = s.scale(c, q, l, u), s.scale(c, q, l, u, quad_diag=d)
    six = s.scale(c, q, l, u, qu, d)
    assert len(four) == 4 and len(five) == 5 and len(six) == 6
    assert all(torch.equal(a, b) for a, b in zip(four, five)) and all(torch.equal(a, b) for a, b in zip(four, six))
    assert five[4].tolist() == [12.0, 2.0] == six[5].tolist() and six[4].tolist() == [8.0, INF, 6.0]
    assert torch.equal(s.scale(c, q, l, u, qu)[4], six[4])


@pytest.mark.parametrize("seed", [1, 2])
def test_half_and_unscaled_kkt_are_invariant_under_the_scaling(seed):
    """h = 1/2 x'Dx and the un-scaled KKT numbers of the scaled problem (K_s = D_row K D_col, c_s = D_col c, d_s = d D_col^2, ...) at
    (x / D_col, y / D_row) equal those of the original problem at (x, y)"""
    qp = make_qp(40, 60, seed)
    rng = np.random.default_rng(seed)
    dc, dr = rng.uniform(0.5, 2.0, qp.n), rng.uniform(0.5, 2.0, qp.m)
    qu = np.where(np.arange(qp.m) % 3 == 0, qp.q + 1.0, INF)
    s = tp.Scaling(torch.from_numpy(dc), torch.from_numpy(dr))
    cs, qs, ls, us, qus, ds = (v.numpy() for v in s.scale(*(torch.from_numpy(v) for v in (qp.c, qp.q, qp.l, qp.u, qu, qp.d))))
    assert np.allclose(ds, qp.d * dc * dc, rtol=1e-15, atol=0)
    A = qp.A.toarray()
    orig, scaled = QuadModel(A, qp.m_ineq, qp.c, qp.q, qp.l, qp.u, qp.d, qu), QuadModel(dr[:, None] * A * dc[None, :], qp.m_ineq, cs, qs, ls, us, ds, qus)
    x, y = rng.standard_normal(qp.n), rng.standard_normal(qp.m)
    xs, ys = x / dc, y / dr
    rel = lambda a, b: abs(a - b) / max(abs(a), abs(b), 1e-300)
    assert orig.half(x) > 1.0 and rel(orig.half(x), scaled.half(xs)) <= 1e-12
    want, got = orig.kkt(x, y, 0.7), scaled.kkt(xs, ys, 0.7, dc, dr)
    for key in want:
        assert rel(want[key], got[key]) <= 1e-12, (key, want[key], got[key])
    sw, lw = orig.sums(x, y)
    sg, lg = scaled.sums(xs, ys, dc, dr)
    assert all(rel(a, b) <= 1e-12 for a, b in zip(sw, sg)) and np.allclose(lw, lg, rtol=1e-12, atol=1e-12)
    # the slots: [3] - h is c'x, [1] + h is l'lam+, and the term matters
    lin = QuadModel(A, qp.m_ineq, qp.c + qp.d * x, qp.q, qp.l, qp.u, None, qu).sums(x, y)[0]      # (same gradient, no h)
    h = orig.half(x)
    assert rel(sw[3] - h, qp.c @ x) <= 1e-12 and rel(sw[1] + h, lin[1]) <= 1e-12 and sw[0] == lin[0] and sw[2] == lin[2]


# ---------------------------------------------------------------------------------------------------
# 3. run_pdlp over the numpy engine
# ---------------------------------------------------------------------------------------------------
MODES = {"fixed": {}, "adaptive": dict(adaptive=True), "halpern": dict(halpern=True)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_run_pdlp_reaches_the_constructed_optimum(seed, mode):
    qp = make_qp(40, 60, seed)
    mo = model_of_qp(qp)
    assert (qp.d == 0).sum() >= 12 and (qp.d > 0).sum() >= 24
    assert abs(mo.objective(qp.xs) - qp.opt) <= 1e-12 * (1 + abs(qp.opt))
    tol = 1e-8
    x, obj, k, n, j, status, _ = run_pdlp(QuadModelEngine(mo), tol=tol, verbose=False, primal_update=True, max_kkt=400_000,
                                          sigma=float(np.linalg.norm(mo.A, 2)), **MODES[mode])
    assert status == "Solved", (status, k)
    assert abs(obj - qp.opt) <= 2e-8 * (1 + 2 * abs(qp.opt)), (obj, qp.opt)
    xv = x.numpy()
    assert (xv >= qp.l).all() and (xv <= qp.u).all()
    assert abs(obj - mo.objective(xv)) <= 1e-9 * (1 + abs(obj))
    # the linear part alone is another number: the term is at work
    assert abs(float(qp.c @ xv) - qp.opt) > 1e-3
    print(f"make_qp(40, 60, {seed}) {mode}: k={k} n={n} j={j} objective {obj:.12g} (opt {qp.opt:.12g})")


# ---------------------------------------------------------------------------------------------------
# 4. d = 0 is the LP
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_all_zero_d_gives_the_trace_of_the_lp(mode):
    qp = make_qp(40, 60, 1)
    lin = QuadModel(qp.A, qp.m_ineq, qp.c + qp.d * qp.xs, qp.q, qp.l, qp.u)          # (the LP with the same optimum x*)
    zero = QuadModel(qp.A, qp.m_ineq, qp.c + qp.d * qp.xs, qp.q, qp.l, qp.u, np.zeros(qp.n))
    traces, outs = [], []
    for mo, quad in ((lin, False), (zero, True)):
        tr = dict(kkt=[], omega=[], restarts=[])
        eng = QuadModelEngine(mo, quad=quad)
        assert (eng.quad_diag is not None) == quad
        outs.append(run_pdlp(eng, tol=1e-8, verbose=False, primal_update=True, max_kkt=400_000, trace=tr,
                             sigma=float(np.linalg.norm(mo.A, 2)), **MODES[mode]))
        traces.append(tr)
    assert outs[0][5] == "Solved" and traces[0] == traces[1] and len(traces[0]["kkt"]) > 10
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1:6] == outs[1][1:6]
