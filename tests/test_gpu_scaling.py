"""One scaling object on every solve path, on the MI355X: ``equilibrate_matrix`` against ``ruiz_precondition``, the full path against
the shard path of a world of one, and the batch's un-scaling against ``Scaling`` -- all bit for bit (nothing here has a tolerance
but the comparison of a batch with ``solve_lp``, which is that of tests/test_gpu_batch.py).

These are structural pins, not independent references: ``ruiz_precondition`` IS ``equilibrate_matrix`` plus ``Scaling.scale``, so the
first two tests hold the thin layers together (shapes, the caller's matrix untouched, nothing lost between them).  That the bits are
those of the code before the three flows were merged is shown by the byte-for-byte dumps of profiles/r11_scaling; the values
themselves are checked against the reference's golden vectors in tests/test_gpu_parity.py::test_ruiz_vs_golden."""
import functools
import os

import numpy as np
import pytest
import torch

import torchpdlp_amd as tp
from tests import test_gpu_pock_chambolle as pct          # the badly scaled 130 x 97 family and same_bits
from torchpdlp_amd.batch import pdlp_algorithm_batch
from torchpdlp_amd.distributed import shard_arrays
from torchpdlp_amd.precondition import ruiz_precondition_shard

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ruiz.npz")
TORCH = {"f32": torch.float32, "f64": torch.float64}
dev, same_bits = pct.dev, pct.same_bits


def golden_cases():
    """the reference's own dense inputs (an all-zero row and column, the Q3 early exit among them): (name, sweeps, c, K, q, l, u) in f32"""
    z = np.load(GOLDEN)
    t = lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=dev())
    for case in sorted({"/".join(k.split("/")[:3]) for k in z.files}):
        r = {k.split("/")[-1]: z[k] for k in z.files if k.startswith(case + "/")}
        yield case, int(case.rsplit("it", 1)[1]), t(r["c"]), tp.CsrPair.from_any(t(r["K"]), device=dev()), t(r["q"]), t(r["l"]), t(r["u"])


def bad_lp(T):
    c, K, q, m_ineq, l, u = pct.single(pct.bad_family(1, TORCH[T]))
    return c, K, q, m_ineq, l, u


def assert_same_equilibration(K, c, q, l, u, what, **kw):
    """``equilibrate_matrix(K)`` gives the bits of ``ruiz_precondition(c, K, q, l, u)`` and leaves ``K`` alone"""
    before, before_t = K.val.clone(), K.t_val.clone()
    want, _, _, _, _, (D_col, D_row, *_), _ = tp.ruiz_precondition(c, K, q, l, u, device=dev(), **kw)
    Ks, sc = tp.equilibrate_matrix(K, device=dev(), **kw)
    assert same_bits(Ks.val, want.val) and same_bits(Ks.t_val, want.t_val), what
    assert sc.d_col.shape == (K.n,) and sc.d_row.shape == (K.m,), what
    assert same_bits(sc.d_col, D_col.view(-1)) and same_bits(sc.d_row, D_row.view(-1)), what
    assert 1 <= sc.sweeps <= kw.get("max_iter", 20) and sc.seconds > 0, what
    assert same_bits(K.val, before) and same_bits(K.t_val, before_t) and Ks.val.data_ptr() != K.val.data_ptr(), what
    return Ks, sc


def test_equilibrate_matrix_is_ruiz_precondition_without_the_vectors():
    n_cases = 0
    for case, it, c, K, q, l, u in golden_cases():
        assert_same_equilibration(K, c, q, l, u, case, max_iter=it)
        n_cases += 1
    assert n_cases >= 8


@pytest.mark.parametrize("T", ["f32", "f64"])
def test_equilibrate_matrix_with_the_pass(T):
    c, K, q, _, l, u = bad_lp(T)
    Ks, _ = assert_same_equilibration(K, c, q, l, u, T, pock_chambolle=True)
    plain, _ = assert_same_equilibration(K, c, q, l, u, T)
    assert not same_bits(Ks.val, plain.val)                       # (the pass did run)


def assert_full_path_is_the_world_1_shard_path(c, K, q, m_ineq, l, u, what, **kw):
    Ks, c_s, q_s, l_s, u_s, (D_col, D_row, *_), _ = tp.ruiz_precondition(c, K, q, l, u, device=dev(), **kw)
    for balance in ("rows", "nnz"):
        sh = shard_arrays(K, c, q, l, u, m_ineq, 0, 1, balance=balance)
        got = ruiz_precondition_shard({k: v for k, v in sh.items() if k != "part"}, None, **kw)
        for key, (rp, ci, va) in (("K_rows", (Ks.rowptr, Ks.colidx, Ks.val)), ("KT_rows", (Ks.t_rowptr, Ks.t_colidx, Ks.t_val))):
            assert torch.equal(got[key][0], rp.long()) and torch.equal(got[key][1], ci.int()), (what, balance, key)
            assert same_bits(got[key][2], va), (what, balance, key)
        for key, want in (("c", c_s), ("q", q_s), ("l", l_s), ("u", u_s), ("d_col", D_col), ("d_row", D_row)):
            assert same_bits(got[key], want.view(-1)), (what, balance, key)
        assert got["ruiz_sweeps"] >= 1 and got["ruiz_seconds"] > 0
        assert same_bits(sh["K_rows"][2], K.val) and same_bits(sh["c"], c.view(-1))      # the shard passed in is untouched


def test_the_full_path_is_the_shard_path_of_one_rank_golden():
    for case, it, c, K, q, l, u in golden_cases():
        assert_full_path_is_the_world_1_shard_path(c, K, q, K.m // 2, l, u, case, max_iter=it)


@pytest.mark.parametrize("T", ["f32", "f64"])
def test_the_full_path_is_the_shard_path_of_one_rank(T):
    assert_full_path_is_the_world_1_shard_path(*bad_lp(T), T)


# ---------------------------------------------------------------------------------------------------------------------------------
# the batch: its scaling and un-scaling are Scaling's
# ---------------------------------------------------------------------------------------------------------------------------------
SOLVE = dict(precondition=True, primal_weight_update=True, adaptive_stepsize=True, seed=0)


@functools.lru_cache(maxsize=None)
def shared_batch():
    f = pct.bad_family(8, torch.float32)
    return f, tp.solve_lp_batch(*pct.batch_args(f), device=dev(), **SOLVE)


def test_batch_over_a_shared_matrix_unscales_through_scaling():
    f, res = shared_batch()
    d = lambda v: v.to(dev())
    Ks, sc = tp.equilibrate_matrix(pct.csr(f), device=dev())
    Xs, Ys, *_ = pdlp_algorithm_batch(Ks, f.m_ineq, *sc.scale(d(f.C), d(f.Q), d(f.L), d(f.U)), dev(), precondition=True,
                                      primal_update=True, adaptive=True, data_precond=(sc.d_col, sc.d_row), seed=0)
    assert same_bits(res.x, sc.unscale_x(Xs)) and same_bits(res.y, sc.unscale_y(Ys))
    assert same_bits(res.x, sc.d_col.view(-1, 1) * Xs) and same_bits(res.y, sc.d_row.view(-1, 1) * Ys)      # ... written out
    assert not same_bits(res.x, Xs)


def test_batch_over_a_shared_matrix_matches_solve_lp():
    """column b against ``solve_lp`` of LP b as tests/test_gpu_batch.py compares them (its bounds)"""
    f, res = shared_batch()
    d = lambda v: v.to(dev())
    for b in range(8):
        one = tp.solve_lp((d(f.C[:, b]), pct.csr(f), d(f.Q[:, b]), f.m_ineq, d(f.L[:, b]), d(f.U[:, b])), device=dev(), **SOLVE)
        print(f"LP {b}: batch {res.status[b]} k = {res.iterations[b]}, solve_lp {one.status} k = {one.iterations}")
        assert res.status[b] == one.status == "Solved", b
        assert abs(res.objective[b] - one.objective) <= 2e-3 * (1 + abs(one.objective)), b
        x, xo = res.x[:, b].double().cpu().numpy(), one.x.view(-1).double().cpu().numpy()
        assert np.linalg.norm(x - xo) <= 2e-2 * (1 + np.linalg.norm(xo)), b


def test_batch_with_a_matrix_per_lp_reports_the_equilibration_alone():
    f = pct.bad_family(8, torch.float32, noise=0.1)
    times = {}
    res = tp.solve_lp_batch(*pct.batch_args(f), device=dev(), K_values=f.vals, setup_times=times, max_kkt=400, **SOLVE)
    print(f"ruiz_seconds {times['ruiz_seconds']:.4f}, time {res.time:.4f}")
    assert 0 < times["ruiz_seconds"] <= res.time
    sv, stv, dc, dr, _ = tp.ruiz_precondition_batch(pct.csr(f), f.vals.to(dev()))
    sc = tp.Scaling(dc, dr)
    d = lambda v: v.to(dev())
    Xs, Ys, *_ = pdlp_algorithm_batch(pct.csr(f), f.m_ineq, *sc.scale(d(f.C), d(f.Q), d(f.L), d(f.U)), dev(), precondition=True,
                                      primal_update=True, adaptive=True, data_precond=(dc, dr), seed=0, K_values=sv, KT_values=stv,
                                      max_kkt=400)
    assert same_bits(res.x, sc.unscale_x(Xs)) and same_bits(res.y, sc.unscale_y(Ys))
