"""CPU checks of batched solves with a constraint matrix per LP over one shared pattern (``solve_lp_batch(K_values=...)``): the
union-pattern helper, the K -> K' permutation, argument validation before any device work, ``gen_lp_family(matrix_noise=...)`` and
the two new entry points' argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import torchpdlp_amd as tp
from torchpdlp_amd import _native as N
from torchpdlp_amd.sparse import csr_transpose, stack_matrices, transpose_perm


def dense_of(pattern, vals):
    K = torch.zeros(pattern.m, pattern.n, dtype=vals.dtype)
    rows = torch.repeat_interleave(torch.arange(pattern.m), pattern.rowptr[1:] - pattern.rowptr[:-1])
    K.index_put_((rows, pattern.colidx.long()), vals, accumulate=True)
    return K


def test_union_pattern_of_dense_matrices_with_missing_entries():
    rng = np.random.default_rng(0)
    mats = []
    for b in range(4):
        K = rng.uniform(0.5, 2.0, (7, 9)) * (rng.random((7, 9)) < 0.4)
        mats.append(torch.from_numpy(K))
    mats[0][2, 3], mats[1][2, 3], mats[2][2, 3], mats[3][2, 3] = 1.5, 0.0, -2.0, 0.0       # an entry two of the four lack
    mats[1][6, :] = 0.0                                                                   # a row one LP lacks altogether
    pattern, vals = stack_matrices(mats)
    union = sum((K != 0) for K in mats) > 0
    assert (pattern.m, pattern.n) == (7, 9) and pattern.nnz == int(union.sum()) and tuple(vals.shape) == (pattern.nnz, 4)
    assert torch.equal(pattern.rowptr, torch.cat([torch.zeros(1, dtype=torch.int64), union.sum(1).cumsum(0)]))
    for i in range(7):                       # columns sorted and distinct inside each row
        cols = pattern.colidx[pattern.rowptr[i]:pattern.rowptr[i + 1]]
        assert (cols[1:] > cols[:-1]).all()
    for b, K in enumerate(mats):
        assert torch.equal(dense_of(pattern, vals[:, b]), K), b
    at = int(pattern.rowptr[2]) + int((pattern.colidx[pattern.rowptr[2]:pattern.rowptr[3]] == 3).nonzero())
    assert vals[at].tolist() == [1.5, 0.0, -2.0, 0.0]                                     # a stored zero where the entry is missing
    assert torch.equal(pattern.val, vals[:, 0])


def test_union_pattern_takes_every_matrix_form_and_refuses_other_shapes():
    sp = pytest.importorskip("scipy.sparse")
    A = torch.tensor([[1.0, 0.0, 2.0], [0.0, 3.0, 0.0]])
    Bm = torch.tensor([[0.0, 5.0, 2.5], [0.0, 3.0, 1.0]])
    forms = [A, Bm.to_sparse(), sp.csr_matrix(A.numpy() * 2), tp.CsrPair.from_dense(Bm * 3)]
    pattern, vals = stack_matrices(forms, dtype=torch.float64)
    for b, K in enumerate((A, Bm, A * 2, Bm * 3)):
        assert torch.equal(dense_of(pattern, vals[:, b]), K.double()), b
    with pytest.raises(ValueError, match="shape"):
        stack_matrices([A, torch.ones(3, 3)])
    with pytest.raises(ValueError):
        stack_matrices([])


@pytest.mark.parametrize("chunk", [1 << 30, 7])
def test_transpose_permutation_against_csr_transpose_of_each_matrix(chunk):
    """t_val = val[perm] for every LP's values, in the order csr_transpose gives -- duplicates and empty rows included, and past
    2^24 positions the integer path stays exact (checked on the position values themselves)"""
    f = tp.gen_lp_family(40, 31, 4, 5, seed=4, dtype=torch.float64, matrix_noise=0.3)
    K = tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val)
    perm = K.transpose_perm()
    assert perm.dtype == torch.int64 and torch.equal(perm, transpose_perm(f.rowptr, f.colidx, f.m, f.n))
    assert torch.equal(torch.sort(perm).values, torch.arange(K.nnz))
    for b in range(f.B):
        rp, ci, tv = csr_transpose(f.rowptr, f.colidx, f.vals[:, b].contiguous(), f.m, f.n, chunk_nnz=chunk)
        assert torch.equal(rp, K.t_rowptr) and torch.equal(ci, K.t_colidx)
        assert torch.equal(f.vals[perm, b], tv), b
        Kb = K.with_values(f.vals[:, b].contiguous(), perm)
        assert torch.equal(Kb.t_val, tv) and Kb.t_colidx is K.t_colidx
    big = torch.arange(K.nnz, dtype=torch.int64) + (1 << 24) + 1             # values float32 cannot hold
    assert torch.equal(csr_transpose(f.rowptr, f.colidx, big, f.m, f.n)[2], big[perm])


def small_problem(B=3):
    f = tp.gen_lp_family(30, 20, 3, B, seed=1, matrix_noise=0.1)
    K = tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val)
    return f, (f.C[:, 0], K, f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0])


def test_matrix_values_are_validated_before_device_work(monkeypatch):
    f, prob = small_problem()
    monkeypatch.setattr(tp.batch, "BatchEngine", None)          # any device work would fail differently
    with pytest.raises(ValueError, match="K_values"):
        tp.solve_lp_batch(prob, f.C, K_values=f.vals[:-1], device="cpu")                 # one stored entry short
    with pytest.raises(ValueError, match="K_values"):
        tp.solve_lp_batch(prob, f.C, K_values=f.vals[:, 0], device="cpu")                # 1-D
    with pytest.raises(ValueError, match="K_values"):
        tp.solve_lp_batch(prob, f.C, K_values=f.vals.unsqueeze(0), device="cpu")
    with pytest.raises(ValueError, match="disagree"):
        tp.solve_lp_batch(prob, f.C, K_values=f.vals[:, :2], device="cpu")               # B of c is 3
    with pytest.raises(ValueError, match="columns"):
        tp.solve_lp_batch(prob, K_values=f.vals, x_init=torch.zeros(f.n, 2), device="cpu")   # B comes from K_values alone
    dense = (f.C[:, 0], tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val).to_dense(), f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0])
    with pytest.raises(ValueError, match="K_values"):                                    # a dense K says its nnz once it is CSR
        tp.solve_lp_batch(dense, f.C, K_values=torch.ones(int((dense[1] != 0).sum()) + 1, 3), device="cpu")


@pytest.mark.parametrize("flag", [dict(comm=True), dict(fishnet=True), dict(precision="mixed"), dict(infeasibility_detect=True),
                                  dict(adaptive_retry=True), dict(direct_exchange=True)])
def test_unsupported_flags_still_raise_with_matrices(flag, monkeypatch):
    f, prob = small_problem()
    monkeypatch.setattr(tp.batch, "BatchEngine", None)
    with pytest.raises(ValueError):
        tp.solve_lp_batch(prob, f.C, K_values=f.vals, device="cpu", **flag)


def test_matrix_noise_zero_is_the_family_as_it_was():
    a = tp.gen_lp_family(60, 45, 4, 5, seed=2)
    b = tp.gen_lp_family(60, 45, 4, 5, seed=2, matrix_noise=0.0)
    assert b.vals is None and a.vals is None and a.opt_obj == b.opt_obj
    for name in ("rowptr", "colidx", "val", "C", "Q", "L", "U", "X_opt", "Y_opt"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # with noise, the draws of x, y, the bounds and the slacks are those of the shared-K family: only K_b, c_b and q_b move
    n = tp.gen_lp_family(60, 45, 4, 5, seed=2, matrix_noise=0.25)
    for name in ("rowptr", "colidx", "val", "L", "U", "X_opt", "Y_opt"):
        assert torch.equal(getattr(a, name), getattr(n, name)), name
    assert not torch.equal(a.C, n.C) and not torch.equal(a.Q, n.Q)


def test_matrix_noise_optima_satisfy_kkt_over_each_matrix():
    """test_gen_lp_family_optima_satisfy_kkt (tests/test_batch_host.py) with K_b in place of K, at its tolerances"""
    f = tp.gen_lp_family(60, 45, 4, 5, seed=2, dtype=torch.float64, matrix_noise=0.3)
    assert tuple(f.vals.shape) == (f.val.numel(), 5) and f.vals.dtype == torch.float64
    ratio = f.vals / f.val.view(-1, 1)
    assert (ratio >= 0.7 - 1e-12).all() and (ratio <= 1.3 + 1e-12).all() and ratio.std() > 0.1
    assert not torch.equal(f.vals[:, 0], f.vals[:, 1])
    for b in range(f.B):
        K = torch.sparse_csr_tensor(f.rowptr, f.colidx.long(), f.vals[:, b], (f.m, f.n)).to_dense().numpy()
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


def test_matrix_noise_family_agrees_with_highs():
    opt = pytest.importorskip("scipy.optimize")
    f = tp.gen_lp_family(40, 30, 4, 4, seed=3, dtype=torch.float64, matrix_noise=0.2)
    for b in range(f.B):
        K = torch.sparse_csr_tensor(f.rowptr, f.colidx.long(), f.vals[:, b], (f.m, f.n)).to_dense().numpy()
        c, q, l, u = (v[:, b].numpy() for v in (f.C, f.Q, f.L, f.U))
        bounds = [(None if np.isinf(a) else a, None if np.isinf(z) else z) for a, z in zip(l, u)]
        h = opt.linprog(c, A_ub=-K[:f.m_ineq], b_ub=-q[:f.m_ineq], A_eq=K[f.m_ineq:], b_eq=q[f.m_ineq:], bounds=bounds, method="highs")
        assert h.status == 0
        assert abs(h.fun - f.opt_obj[b]) <= 1e-6 * (1 + abs(f.opt_obj[b]))


def test_new_entry_points_reject_null_arguments_without_a_gpu():
    lib = N.load()
    assert {"pdlp_batch_attach_matrices", "pdlp_batch_product"} <= set(N.SIGNATURES)
    b = N.PdlpBatch()
    one = C.c_void_p(64)                     # never dereferenced: the checks come first
    assert lib.pdlp_batch_attach_matrices(None, 8, one, one, None, None) == -1
    assert lib.pdlp_batch_attach_matrices(None, 8, None, None, None, None) == -1
    assert lib.pdlp_batch_product(None, C.byref(b), 0, one, C.c_void_p(128)) == -1
    assert lib.pdlp_batch_product(None, None, 0, one, C.c_void_p(128)) == -1
    assert lib.pdlp_batch_product(None, C.byref(b), 0, None, one) == -1
    assert lib.pdlp_batch_product(None, C.byref(b), 1, one, None) == -1


def test_algorithm_refuses_values_of_another_shape(monkeypatch):
    """pdlp_algorithm_batch's own check, reached before it creates anything on a device"""
    f, _ = small_problem()
    K = tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val)
    monkeypatch.setattr(tp.batch, "PdlpEngine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    with pytest.raises(ValueError, match="K_values"):
        tp.batch.pdlp_algorithm_batch(K, f.m_ineq, f.C, f.Q, f.L, f.U, "cpu", K_values=f.vals[1:])
    with pytest.raises(ValueError, match="disagree"):
        tp.batch.pdlp_algorithm_batch(K, f.m_ineq, f.C, f.Q, f.L, f.U, "cpu", K_values=f.vals[:, :2])
