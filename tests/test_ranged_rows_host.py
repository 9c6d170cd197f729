"""Two-sided constraint rows on the host (no GPU): the MPS reader that keeps a RANGES row as one row, the validation of ``q_upper``
and every refusal before device work, and ``run_pdlp`` over a float64 numpy engine that implements the two-sided arithmetic
(tests/ranged_model.py) -- the norm the termination test is handed, and a whole solve against the split twin."""
import os

import numpy as np
import pytest
import torch

import torchpdlp_amd as tp
from tests.ranged_model import RangedModel, RangedModelEngine, feasible_ranged_lp, split_model
from torchpdlp_amd import _native as N
from torchpdlp_amd import solver
from torchpdlp_amd.ranged import check_row_upper, norm_vector, split_rows
from torchpdlp_amd.solver import pdlp_algorithm, run_pdlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGED = os.path.join(ROOT, "tests", "golden", "ranged", "ranged.mps")
INF = float("inf")


# ---------------------------------------------------------------------------------------------------
# the reader
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_ranged_form_is_the_split_form_without_the_second_rows(dtype):
    c, K, q, m_ineq, l, u = tp.mps_to_standard_form(RANGED, dtype=dtype)
    cr, Kr, qr, mr, lr, ur, qur = tp.mps_to_ranged_form(RANGED, dtype=dtype)
    # the fixture: R01 (G), R02 (L), R03 (E, R > 0), R04 (E, R < 0) are ranged -> pairs at rows 0..7 of the split form; the other
    # inequality rows R05, R06, R08, R09, R11, R12 follow, then the equality rows R07, R10
    assert (K.m, m_ineq, Kr.m, mr) == (16, 14, 12, 10)
    second = [1, 3, 5, 7]
    keep = [i for i in range(K.m) if i not in second]
    dense = lambda P: torch.sparse_csr_tensor(P.rowptr, P.colidx.long(), P.val, size=(P.m, P.n)).to_dense()
    Kd, Krd = dense(K), dense(Kr)
    assert torch.equal(Krd, Kd[keep]) and torch.equal(qr, q[keep])
    assert torch.equal(Kd[second], -Kd[[0, 2, 4, 6]])                   # (each second row is the negated first)
    assert all(torch.equal(a, b) for a, b in ((cr, c), (lr, l), (ur, u)))
    want = torch.full((12, 1), INF, dtype=dtype)
    want[[0, 1, 2, 3]] = -q[second]
    assert torch.equal(qur, want)
    # the four kinds, as numbers: G [2, 5]; L [4, 8]; E with R = 2 [3, 5]; E with R = -2 [4, 6]
    assert qr[:4].view(-1).tolist() == [2.0, 4.0, 3.0, 4.0] and qur[:4].view(-1).tolist() == [5.0, 8.0, 5.0, 6.0]
    assert (Kr.rowptr.dtype, Kr.colidx.dtype, Kr.val.dtype) == (torch.int64, torch.int32, dtype)
    check_row_upper(qr, qur, mr)                                         # what the reader returns is valid input
    # split_rows puts the second rows back where the reader of the split form has them
    import scipy.sparse as sp
    As, qs, mi, first = split_rows(sp.csr_matrix(Krd.double().numpy()), qr.view(-1).double().numpy(), qur.view(-1).double().numpy(), mr)
    assert mi == m_ineq and np.array_equal(As.toarray(), Kd.double().numpy()) and np.array_equal(qs, q.view(-1).double().numpy())


def test_standard_form_reads_as_before():
    """afiro has no RANGES: both readers give the same problem, q_upper all +inf"""
    afiro = os.path.join(ROOT, "tests", "golden", "mps", "afiro.mps")
    a, b = tp.mps_to_standard_form(afiro), tp.mps_to_ranged_form(afiro)
    assert all(torch.equal(x, y) for x, y in zip((a[0], a[2], a[4], a[5], a[1].val, a[1].colidx, a[1].rowptr),
                                                 (b[0], b[2], b[4], b[5], b[1].val, b[1].colidx, b[1].rowptr)))
    assert a[3] == b[3] and bool(torch.isinf(b[6]).all()) and b[6].shape == a[2].shape


# ---------------------------------------------------------------------------------------------------
# validation and refusals, all before device work
# ---------------------------------------------------------------------------------------------------
K3 = torch.eye(3)
V3 = torch.zeros(3)
BAD = {"length": [1.0, 2.0], "below_q": [-1.0, INF, INF], "nan": [float("nan"), INF, INF], "minus_inf": [-INF, INF, INF],
       "equality_row_other": [INF, INF, 5.0], "2d_wrong_length": [[1.0], [2.0]]}


@pytest.mark.parametrize("name", list(BAD))
def test_malformed_q_upper_raises_before_any_device_work(name):
    qu = torch.tensor(BAD[name])
    with pytest.raises(ValueError, match="q_upper"):
        pdlp_algorithm(K3, 2, V3, V3, V3, V3 + 1, "cpu", verbose=False, q_upper=qu)
    with pytest.raises(ValueError, match="q_upper"):
        tp.solve_lp((V3, K3, V3, 2, V3, V3 + 1), device="cpu", q_upper=qu)


def test_well_formed_q_upper_passes_the_check():
    q = torch.tensor([1.0, -2.0, 3.0, 4.0])
    for ok in ([INF, INF, INF, INF], [1.0, 0.0, INF, 4.0], [2.0, -2.0, INF, INF]):
        out = check_row_upper(q.view(-1, 1), torch.tensor(ok).view(-1, 1), 2)
        assert out.shape == (4,) and out.dtype == q.dtype
    assert check_row_upper(q, None, 2) is None
    with pytest.raises(ValueError, match="finite"):
        check_row_upper(torch.tensor([-INF, 0.0]), torch.tensor([1.0, INF]), 1)     # rows with q = -inf are out of scope
    # ... and then reaches the device: on a machine without one, or with device="cpu", that is the first failure
    with pytest.raises(Exception) as e:
        tp.solve_lp((V3, K3, V3, 2, V3, V3 + 1), device="cpu", q_upper=torch.tensor([1.0, INF, INF]))
    assert not isinstance(e.value, ValueError)


REFUSED = [dict(precision="mixed"), dict(comm=True), dict(infeasibility_detect=True), dict(adaptive=True, adaptive_retry=True),
           dict(fishnet=True)]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: "+".join(kw))
def test_refused_combinations_raise_before_any_device_work(kw):
    qu = torch.tensor([1.0, INF, INF])
    names = dict(adaptive="adaptive_stepsize")
    with pytest.raises(ValueError, match="q_upper"):
        tp.solve_lp((V3, K3, V3, 2, V3, V3 + 1), device="cpu", q_upper=qu, **{names.get(k, k): v for k, v in kw.items()})
    with pytest.raises(ValueError, match="q_upper"):
        tp.solve_lp(RANGED, device="cpu", ranged_rows=True, **{names.get(k, k): v for k, v in kw.items()})
    if "fishnet" not in kw:                            # (fishnet is solve_lp's flag)
        with pytest.raises(ValueError, match="q_upper"):
            pdlp_algorithm(K3, 2, V3, V3, V3, V3 + 1, "cpu", verbose=False, q_upper=qu, **kw)


def test_ranged_rows_flag_needs_a_path_and_the_batch_has_no_keyword():
    with pytest.raises(ValueError, match="ranged_rows"):
        tp.solve_lp((V3, K3, V3, 2, V3, V3 + 1), device="cpu", ranged_rows=True)
    with pytest.raises(TypeError, match="q_upper"):
        tp.solve_lp_batch((V3, K3, V3, 2, V3, V3 + 1), device="cpu", q_upper=torch.tensor([1.0, INF, INF]))


def test_driver_refuses_too():
    """run_pdlp / PdhgDriver over an engine that has q_upper: the same refusals, before the engine is used"""
    class Engine:
        comm, mixed, delta, q_upper, m_ineq = None, False, False, torch.tensor([1.0]), 1
        dtype = torch.float32

        def __getattr__(self, name):
            raise AssertionError(f"engine.{name} was used")
    for kw in (dict(infeasibility_detect=True), dict(adaptive=True, adaptive_retry=True)):
        with pytest.raises(ValueError, match="q_upper"):
            run_pdlp(Engine(), verbose=False, sigma=1.0, **kw)


def test_library_entry_point_and_cli_flag():
    lib = N.load()
    assert "pdlp_set_row_upper" in N.SIGNATURES and N.ABI_VERSION == 18 == lib.pdlp_abi_version()
    assert lib.pdlp_set_row_upper(None, None) == -1
    from torchpdlp_amd.__main__ import parse_args
    assert parse_args(["--ranged_rows"]).ranged_rows is True and parse_args([]).ranged_rows is False


def test_scaling_scales_q_upper_like_q():
    s = tp.Scaling(torch.tensor([2.0, 0.5]), torch.tensor([4.0, 0.25, 2.0]))
    c, q, l, u = torch.ones(2), torch.tensor([1.0, -2.0, 3.0]), torch.zeros(2), torch.ones(2)
    four = s.scale(c, q, l, u)
    five = s.scale(c, q, l, u, torch.tensor([2.0, INF, 3.0]))
    assert len(four) == 4 and len(five) == 5 and all(torch.equal(a, b) for a, b in zip(four, five))
    assert five[4].tolist() == [8.0, INF, 6.0] and four[1].tolist() == [4.0, -0.5, 6.0]


def test_norm_vector():
    q, qu = torch.tensor([3.0, -4.0, 1.0, -2.0, 5.0]), torch.tensor([INF, -1.0, 7.0, -2.0, INF])
    assert norm_vector(q, None, 4) is q
    assert norm_vector(q, qu, 4).tolist() == [3.0, 4.0, 7.0, 2.0, 5.0]
    assert norm_vector(q, torch.tensor([INF, -1.0, 7.0, INF, 9.0]), 3).tolist() == [3.0, 4.0, 7.0, -2.0, 5.0]     # (equality rows: q)


# ---------------------------------------------------------------------------------------------------
# run_pdlp over the numpy engine
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lp():
    return feasible_ranged_lp(60, 45, 4, seed=2)


@pytest.mark.parametrize("halpern", [False, True], ids=["pdhg", "halpern"])
def test_run_pdlp_solves_the_two_sided_lp_like_its_split_twin(lp, halpern, monkeypatch):
    A, m_ineq, c, q, l, u, qu = lp
    mo = RangedModel(A, m_ineq, c, q, l, u, qu)
    assert np.isfinite(qu[:m_ineq]).sum() >= 20 and (qu[:m_ineq] == q[:m_ineq]).sum() >= 5
    seen = []
    real = solver.terminated
    monkeypatch.setattr(solver, "terminated", lambda res, qn, cn, tol, t=np.float32: seen.append((qn, cn)) or real(res, qn, cn, tol, t))
    tol, sigma = 1e-6, float(np.linalg.norm(mo.A, 2))
    kw = dict(tol=tol, verbose=False, primal_update=True, sigma=sigma, halpern=halpern, max_kkt=2_000_000)
    x, obj, k, n, j, status, _ = run_pdlp(RangedModelEngine(mo), **kw)
    assert status == "Solved", (status, k)
    # the norm handed to the termination test: max(|q_i|, |q_upper_i|) on the two-sided rows, not ||q||
    two = (np.arange(mo.m) < m_ineq) & np.isfinite(qu)
    want = float(np.linalg.norm(np.where(two, np.maximum(np.abs(q), np.abs(qu)), q)))
    assert seen and all(float(qn) == np.float64(want) and float(cn) == float(np.linalg.norm(c)) for qn, cn in seen)
    assert want != float(np.linalg.norm(q)) and abs(mo.norm_q() - want) <= 1e-12 * want
    # the point: inside the bounds, both sides of every row within tol, and the split twin's objective
    xv = x.numpy()
    kx = mo.A @ xv
    assert (xv >= l).all() and (xv <= u).all()
    viol = np.concatenate([np.minimum(kx - q, 0)[:m_ineq], np.maximum(kx - qu, 0)[:m_ineq], (kx - q)[m_ineq:]])
    assert np.linalg.norm(viol) <= tol * (1 + want)
    seen.clear()
    sp_mo = split_model(mo)
    xs, obj_s, ks, _, _, status_s, _ = run_pdlp(RangedModelEngine(sp_mo, q_upper=False), **kw)
    assert status_s == "Solved"
    assert all(float(qn) == float(np.linalg.norm(sp_mo.q)) for qn, _ in seen)               # (no q_upper: today's norm)
    r = mo.kkt(xv, np.zeros(mo.m), 1.0)
    assert abs(obj - obj_s) <= 2 * tol * (1 + 2 * abs(obj_s)), (obj, obj_s)
    assert abs(obj - r["p"]) <= 1e-9 * (1 + abs(obj))
    print(f"two-sided {mo.m} rows: k={k}; split {sp_mo.m} rows: k={ks}; objective {obj:.9g} / {obj_s:.9g}")


def test_model_engine_treats_all_infinite_q_upper_as_no_q_upper(lp):
    """the model itself: +inf everywhere is the one-sided step and the one-sided sums, exactly"""
    A, m_ineq, c, q, l, u, _ = lp
    a, b = RangedModel(A, m_ineq, c, q, l, u, np.full(A.shape[0], INF)), RangedModel(A, m_ineq, c, q, l, u)
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal(a.n), rng.standard_normal(a.m)
    for mo in (a, b):
        xc, yc, _, _ = mo.step(x, y, 0.1, 0.2)
        one = y + 0.2 * (q - mo.A @ (xc + (xc - x)))
        one[:m_ineq] = np.maximum(one[:m_ineq], 0)
        assert np.array_equal(yc, one)
    assert a.kkt(x, y, 0.7) == b.kkt(x, y, 0.7)
