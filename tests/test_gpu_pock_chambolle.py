"""The Pock-Chambolle pass after Ruiz (``pock_chambolle=True``) on the MI355X: the factor kernel (pdlp_csr_row_l1_factors) alone,
the whole preconditioner, a solve, the batch's bit-identities and the CLI.  The reference has no such pass: the yardstick is float64
numpy written here.

u is the unit roundoff of the working precision T (2^-24, 2^-53); 1 ulp of a T number is ``np.spacing`` of it.
"""
import csv
import os
import shutil

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import torchpdlp_amd as tp
from tests import test_gpu_report as rp           # the report tests' float64 reference and its bound (test 3)
from torchpdlp_amd import _native as N
from torchpdlp_amd import precondition as pc
from torchpdlp_amd.engine import _DT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AFIRO = os.path.join(ROOT, "tests", "golden", "mps", "afiro.mps")
AFIRO_OPT = -464.7531428571
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
UNIT = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
IVIEW = {torch.float32: torch.int32, torch.float64: torch.int64}
DTYPES = pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])


def dev():
    return torch.device("cuda", 0)


def h64(t):
    return t.detach().cpu().double().numpy().reshape(-1)


def same_bits(a, b):
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(IVIEW[a.dtype]), b.contiguous().view(IVIEW[b.dtype]))
    if isinstance(a, (list, str)):
        return a == b
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the factor kernel alone
# ---------------------------------------------------------------------------------------------------------------------------------
def l1_factors(rowptr, val, rows):
    """pdlp_csr_row_l1_factors on device arrays; the output starts as NaN, so a row the kernel skips shows"""
    out = torch.full((rows,), float("nan"), dtype=val.dtype, device=dev())
    stream = torch.cuda.current_stream(dev())
    N.check(N.load().pdlp_csr_row_l1_factors(_DT[val.dtype], rows, rowptr.data_ptr(), val.data_ptr(), out.data_ptr(), stream.cuda_stream),
            "pdlp_csr_row_l1_factors")
    stream.synchronize()
    return out


def check_factors(got, sums, L, T, what):
    """``got`` against sqrt(sums) (float64 numpy) cast to T: the kernel's double sum of L terms is off by at most (L - 1) 2^-53
    relative, then one sqrt and one rounding to T -- 1 ulp in float32, (L + 2) 2^-53 relative in float64; a zero sum gives exactly 1"""
    got = got.cpu().numpy()
    assert got.dtype == T and np.isfinite(got).all(), what
    zero = sums == 0
    assert (got[zero] == 1).all(), what
    want = np.sqrt(sums[~zero])
    g = got[~zero].astype(np.float64)
    if T == np.float32:
        w32 = want.astype(np.float32)
        err, allow = np.abs(g - w32.astype(np.float64)), np.spacing(w32).astype(np.float64)
    else:
        err, allow = np.abs(g - want), (L[~zero] + 2) * 2.0 ** -53 * want
    print(f"{what}: max error / bound = {float(np.max(err / allow, initial=0.0)):.3g}")
    assert (err <= allow).all(), what


def factors_of_csr(A, K64, T):
    """row factors from the CSR copy of K64 and column factors from the K' copy, each call made twice"""
    A.sort_indices()
    Kp = tp.CsrPair(A.shape[0], A.shape[1], torch.from_numpy(A.indptr.astype(np.int64)), torch.from_numpy(A.indices.astype(np.int32)),
                    torch.from_numpy(A.data.astype(T))).to(dev())
    out = []
    for rp_, va, rows, axis, L in ((Kp.rowptr, Kp.val, Kp.m, 1, np.diff(A.indptr)),
                                  (Kp.t_rowptr, Kp.t_val, Kp.n, 0, np.bincount(A.indices, minlength=A.shape[1]))):
        first, again = l1_factors(rp_, va, rows), l1_factors(rp_, va, rows)
        assert same_bits(first, again)
        check_factors(first, np.abs(K64).sum(axis=axis), L.astype(np.float64), T, f"{np.dtype(T).name} axis {axis}")
        out.append(first)
    return out


@DTYPES
def test_factors_of_rows_on_both_sides_of_a_lane_group_and_a_wave(T):
    lengths = [0, 1, 7, 8, 9, 63, 64, 65, 300]
    rng = np.random.default_rng(1)
    K64 = np.zeros((len(lengths), 300))
    for i, ln in enumerate(lengths):
        cols = np.sort(rng.choice(300, ln, replace=False))
        K64[i, cols] = (rng.uniform(0.2, 2.0, ln) * rng.choice([-1, 1], ln)).astype(T)
    A = sp.csr_matrix(K64)
    assert list(np.diff(A.indptr)) == lengths
    r, c = factors_of_csr(A, K64, T)
    assert float(r[0]) == 1.0                                     # the empty row


@DTYPES
def test_factors_of_a_matrix_with_an_empty_column_and_a_row_of_stored_zeros(T):
    m, n = 130, 97
    rng = np.random.default_rng(2)
    live = np.setdiff1d(np.arange(n), [5])
    rows = np.repeat(np.arange(m), 5)
    cols = np.concatenate([np.sort(rng.choice(live, 5, replace=False)) for _ in range(m)])
    vals = (rng.uniform(0.2, 2.0, rows.size) * rng.choice([-1, 1], rows.size)).astype(T).astype(np.float64)
    vals[rows == 7] = 0.0                                         # stored zeros: the sum is 0, the factor 1
    A = sp.csr_matrix((vals, cols, np.arange(0, 5 * m + 1, 5)), shape=(m, n))
    assert A.nnz == 5 * m                                         # (the zeros stay stored)
    K64 = A.toarray()
    assert (vals < 0).any() and (vals > 0).any()
    r, c = factors_of_csr(A, K64, T)
    assert float(r[7]) == 1.0 and float(c[5]) == 1.0 and len(set(r.cpu().tolist())) > 100


# ---------------------------------------------------------------------------------------------------------------------------------
# the badly scaled family: 130 x 97, 5 per row, rows and columns multiplied by 10^U(-2, 2); the optima are those of the family
# ---------------------------------------------------------------------------------------------------------------------------------
def bad_family(B, dtype, noise=0.0, seed=5):
    """``diag(R) K diag(S)`` over ``tp.gen_lp_family``'s K with ``x = x0 / S``, ``y = y0 / R``: c' = S c, q' = R q, the bounds / S,
    the objective and the optimal pair unchanged (built in float64, then rounded to ``dtype``)"""
    f = tp.gen_lp_family(97, 130, 5, B, seed=seed, dtype=torch.float64, matrix_noise=noise)
    rng = np.random.default_rng(17)
    R = torch.from_numpy(10.0 ** rng.uniform(-2, 2, f.m)).view(-1, 1)
    S = torch.from_numpy(10.0 ** rng.uniform(-2, 2, f.n)).view(-1, 1)
    rows = torch.repeat_interleave(torch.arange(f.m), torch.diff(f.rowptr))
    s = (R.view(-1)[rows] * S.view(-1)[f.colidx.long()])
    f.val = (f.val * s).to(dtype)
    if f.vals is not None:
        f.vals = (f.vals * s.view(-1, 1)).to(dtype).contiguous()
    f.C, f.Q, f.L, f.U = (f.C * S).to(dtype), (f.Q * R).to(dtype), (f.L / S).to(dtype), (f.U / S).to(dtype)
    f.X_opt, f.Y_opt = f.X_opt / S, f.Y_opt / R
    return f


def csr(f, vals=None):
    K = tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val)
    return (K if vals is None else K.with_values(vals.contiguous())).to(dev())


def single(f, b=0):
    d = lambda v: v[:, b].to(dev())
    return d(f.C), csr(f), d(f.Q), f.m_ineq, d(f.L), d(f.U)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the whole preconditioner
# ---------------------------------------------------------------------------------------------------------------------------------
def returned_tensors(out):
    Ks, c_s, q_s, l_s, u_s, dp, _ = out
    return [Ks.val, Ks.t_val, c_s, q_s, l_s, u_s, dp[0], dp[1]]


@DTYPES
def test_ruiz_then_the_pass(T, monkeypatch):
    """An entry of the scaled matrix went through two divisions per Ruiz sweep and two in the pass, its factors through one rounding
    per sweep and one in the pass each: ``|Ks_ij - D_row_i K_ij D_col_j| <= (2 s + 4) u |D_row_i K_ij D_col_j|`` with s sweeps run,
    the right-hand side in float64; both copies.  The composed factors are the Ruiz-only factors of the same call divided by the
    pass's r, c (float64 numpy from the Ruiz-only matrix) to 2 ulp.  Without the flag nothing changes: the same bits."""
    f = bad_family(1, TORCH[T])
    c, K, q, _, l, u = single(f)
    sweeps = []
    run = pc._sweeps
    monkeypatch.setattr(pc, "_sweeps", lambda *a, **k: sweeps.append(run(*a, **k)) or sweeps[-1])
    base = tp.ruiz_precondition(c, K, q, l, u, device=dev())
    off = tp.ruiz_precondition(c, K, q, l, u, device=dev(), pock_chambolle=False)
    on = tp.ruiz_precondition(c, K, q, l, u, device=dev(), pock_chambolle=True)
    for a, b in zip(returned_tensors(base), returned_tensors(off)):
        assert same_bits(a, b)
    assert torch.equal(K.val, csr(f).val)                         # the caller's matrix is untouched
    s = sweeps[-1]
    assert len(sweeps) == 3 and sweeps[0] == s and 1 <= s <= 20
    Ks, Dc, Dr = on[0], h64(on[5][0]), h64(on[5][1])
    assert not same_bits(Ks.val, off[0].val)
    krows = np.repeat(np.arange(f.m), np.diff(h64(K.rowptr).astype(np.int64)))
    kcols = h64(K.colidx).astype(np.int64)
    trows = np.repeat(np.arange(f.n), np.diff(h64(K.t_rowptr).astype(np.int64)))          # rows of K': variables
    tcols = h64(K.t_colidx).astype(np.int64)                                               # columns of K': constraints
    for name, got, orig, ri, ci in (("K", Ks.val, K.val, krows, kcols), ("K'", Ks.t_val, K.t_val, tcols, trows)):
        want = Dr[ri] * h64(orig) * Dc[ci]
        err, allow = np.abs(h64(got) - want), (2 * s + 4) * UNIT[T] * np.abs(want)
        print(f"{np.dtype(T).name} {name}: {s} sweeps, max error / bound = {float(np.max(err / allow)):.3g}")
        assert (err <= allow).all(), name
    # the vectors carry the composed factors (enhancements.py:64-67 with them)
    assert same_bits(on[1].view(-1), c * on[5][0].view(-1)) and same_bits(on[2].view(-1), q * on[5][1].view(-1))
    assert same_bits(on[3].view(-1), l / on[5][0].view(-1)) and same_bits(on[4].view(-1), u / on[5][0].view(-1))
    # D = D_ruiz / (r, c), r and c of the Ruiz-only matrix
    A = np.zeros((f.m, f.n))
    np.add.at(A, (krows, kcols), np.abs(h64(off[0].val)))
    one_if_zero = lambda v: np.where(v == 0, 1.0, v)
    r = np.sqrt(one_if_zero(A.sum(axis=1))).astype(T).astype(np.float64)
    cc = np.sqrt(one_if_zero(A.sum(axis=0))).astype(T).astype(np.float64)
    for name, got, ruiz, fac in (("D_row", Dr, h64(off[5][1]), r), ("D_col", Dc, h64(off[5][0]), cc)):
        want = ruiz / fac
        ulp = np.spacing(np.abs(want).astype(T)).astype(np.float64)
        print(f"{np.dtype(T).name} {name}: max error = {float(np.max(np.abs(got - want) / ulp)):.3g} ulp")
        assert (np.abs(got - want) <= 2 * ulp).all(), name


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. a solve
# ---------------------------------------------------------------------------------------------------------------------------------
def test_solve_lp_with_the_pass_returns_the_original_problems_solution():
    f = bad_family(1, torch.float64)
    problem = single(f)
    c, K, q, m_ineq, l, u = problem
    res = tp.solve_lp(problem, device=dev(), tol=1e-6, precondition=True, pock_chambolle=True, primal_weight_update=True,
                      adaptive_stepsize=True, dtype=torch.float64, seed=0, max_kkt=2_000_000)
    print(f"status {res.status}, k = {res.iterations}, objective {res.objective!r}, optimum {f.opt_obj[0]!r}, {res.time:.2f} s")
    assert res.status == "Solved"
    x, y = h64(res.x), h64(res.y)
    # x = D_col x_s with x_s inside [l / D_col, u / D_col]: two roundings -- and the returned x_s may be a restart candidate, the
    # step-weighted average of up to k iterates (each inside the box) accumulated in T, one rounding per term.  A wrong or missing
    # factor would be off by the factor itself (D_col spans four decades here)
    eps = np.finfo(np.float64).eps
    lo, hi = h64(l), h64(u)
    out = np.maximum(np.maximum(lo - x, x - hi), 0.0)
    print(f"largest bound violation {out.max():.3e} at |x| = {np.abs(x[out.argmax()]):.3e}")
    assert (out <= (res.iterations + 4) * eps * np.abs(x)).all()
    assert abs(float(h64(c) @ x) - res.objective) <= 1e-9 * (1 + np.abs(h64(c) * x).sum())          # x is the ORIGINAL problem's point
    assert abs(res.objective - f.opt_obj[0]) <= 2e-3 * (1 + abs(f.opt_obj[0]))       # (tests/test_gpu_batch.py, the Ruiz solves)
    # the report's residuals from x, y and the original K in float64 numpy, to the bound of tests/test_gpu_report.py; an entry of
    # the scaled matrix carries the pass's two divisions on top of the sweeps'
    P, _ = rp.original_problem(problem, torch.float64)
    u64 = rp.U64
    _, _, s, _, _, b = rp.ref_report(P, x, y, 0, u64, extra=rp.RUIZ_ROUNDINGS + 2)
    root = lambda v, e: (np.sqrt(v), min(np.sqrt(rp.C_BOUND * e), e / max(np.sqrt(v), 1e-300)) + u64 * np.sqrt(v))
    for name, (want, e) in (("primal_residual", root(s[4], b[4])), ("dual_residual", root(s[0], b[0]))):
        print(f"{name}: reported {getattr(res, name)!r}, float64 numpy {want!r}")
        rp.assert_within(getattr(res, name), want, e + u64 * abs(want), name)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the batch
# ---------------------------------------------------------------------------------------------------------------------------------
REPORT_FIELDS = ("reduced_costs", "row_activity", "dual_objective", "primal_residual", "dual_residual", "gap", "rel_primal_residual",
                 "rel_dual_residual", "rel_gap")


def assert_same_batch(a, b, cols_a=None, cols_b=None, what=""):
    """x, y, the objective, the counters, the status and every report field of the chosen LPs: the same bits"""
    def pick(v, cols):
        if cols is None:
            return v
        return [v[i] for i in cols] if isinstance(v, list) else v[..., cols]
    for name in ("x", "y", "objective", "iterations", "restarts", "kkt_passes", "status") + REPORT_FIELDS:
        va, vb = getattr(a, name), getattr(b, name)
        assert va is not None and same_bits(pick(va, cols_a), pick(vb, cols_b)), f"{what}: {name}"


BATCH = dict(precondition=True, pock_chambolle=True, primal_weight_update=True, adaptive_stepsize=True, seed=0, group_width=8,
             max_kkt=4000)


def batch_args(f, cols=None):
    cols = list(range(f.B)) if cols is None else cols
    prob = (f.C[:, cols[0]], csr(f), f.Q[:, cols[0]], f.m_ineq, f.L[:, cols[0]], f.U[:, cols[0]])
    return prob, f.C[:, cols], f.Q[:, cols], f.L[:, cols], f.U[:, cols]


def test_batch_over_a_shared_matrix_equals_equal_columns_of_values(monkeypatch):
    """The step size is pinned, as the bit-identity tests of tests/test_gpu_batch_matrices.py pin it (``sigma=``): a shared K takes
    it from the single-LP power iteration and ``K_values`` from the batched one, two summation orders whose estimates differ in the
    last digits with or without the pass (3.0928428 against 3.0928426 on this matrix with Ruiz alone).  Everything else of the two
    calls is compared as it runs: the pass once against the pass per LP, the scaling of every column, the solve, the report."""
    f = bad_family(8, torch.float32)
    Ks = tp.equilibrate_matrix(csr(f), device=dev(), pock_chambolle=True)[0]
    dense = np.zeros((f.m, f.n))
    np.add.at(dense, (np.repeat(np.arange(f.m), 5), h64(Ks.colidx).astype(np.int64)), h64(Ks.val))
    sigma = float(np.linalg.norm(dense, 2))
    monkeypatch.setattr(tp.batch, "estimate_sigma", lambda eng, *a, **k: sigma)
    monkeypatch.setattr(tp.batch, "estimate_sigma_batch", lambda be, *a, **k: np.full(be.B, sigma))
    a = tp.solve_lp_batch(*batch_args(f), device=dev(), **BATCH)
    b = tp.solve_lp_batch(*batch_args(f), device=dev(), K_values=f.val.view(-1, 1).repeat(1, 8), **BATCH)
    print("iterations", list(a.iterations), "status", sorted(set(a.status)))
    assert int(a.iterations.max()) >= 80 and len(a) == 8
    assert_same_batch(a, b, what="shared K against K_values")


def test_an_lp_with_its_own_matrix_does_not_depend_on_its_column():
    f = bad_family(8, torch.float32, noise=0.1)
    assert not torch.equal(f.vals[:, 0], f.vals[:, 1])
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    a = tp.solve_lp_batch(*batch_args(f), device=dev(), K_values=f.vals, **BATCH)
    b = tp.solve_lp_batch(*batch_args(f, perm), device=dev(), K_values=f.vals[:, perm], **BATCH)
    assert int(a.iterations.max()) >= 80
    assert_same_batch(a, b, cols_a=perm, cols_b=list(range(8)), what="another column")


def test_streamed_family_equals_the_plain_batch():
    f = bad_family(24, torch.float32)
    a = tp.solve_lp_batch(*batch_args(f), device=dev(), **BATCH)
    sched = {}
    b = tp.solve_lp_batch(*batch_args(f), device=dev(), slots=8, schedule=sched, **BATCH)
    assert sched["slots"] == 8 and sched["admitted_at"].max() > 0 and len(b) == 24
    assert_same_batch(a, b, what="slots=8 against the plain batch")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the CLI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_with_the_pass_solves_afiro(tmp_path):
    from torchpdlp_amd.__main__ import main
    one = tmp_path / "in"
    one.mkdir()
    shutil.copy(AFIRO, one / "afiro.mps")
    rc = main(["--instance_path", str(one), "--output_path", str(tmp_path / "out"), "--adaptive_stepsize", "--primal_weight_update",
               "--precondition", "--pock_chambolle", "--seed", "1", "--max_kkt", "200000"])
    assert rc == 0
    row = list(csv.DictReader(open(tmp_path / "out" / "solver_results.csv")))[0]
    print(row)
    assert row["Status"] == "Solved" and abs(float(row["Objective"]) - AFIRO_OPT) < 0.5      # (test_cli_writes_the_reference_csv_schema)
    # the flag without --precondition is the solver's ValueError: a failure row, as the driver records every failure
    rc = main(["--instance_path", str(one), "--output_path", str(tmp_path / "out2"), "--pock_chambolle"])
    row = list(csv.DictReader(open(tmp_path / "out2" / "solver_results.csv")))[0]
    assert rc == 0 and row["Status"].startswith("Solver failed") and "pock_chambolle" in row["Status"]
