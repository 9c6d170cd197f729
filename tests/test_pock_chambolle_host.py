"""CPU checks of the Pock-Chambolle pass (``pock_chambolle=True``): the argument rules of ``solve_lp`` / ``solve_lp_batch`` hold before
any device work, the CLI takes the flag, and the C ABI has the factor entry point."""
import types

import pytest
import torch

import torchpdlp_amd as tp
from torchpdlp_amd import _native as N


def small_problem(B=3):
    f = tp.gen_lp_family(30, 20, 3, B, seed=1)
    K = tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val)
    return f, (f.C[:, 0], K, f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0])


def no_device_work(monkeypatch):
    """anything past the argument checks fails differently"""
    def never(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(tp.batch, "BatchEngine", None)
    for name in ("load_problem", "ruiz_precondition", "equilibrate_matrix", "ruiz_precondition_batch", "pdlp_algorithm",
                 "_solve_lp_sharded", "resolve_device"):
        monkeypatch.setattr(tp.api, name, never)


def test_solve_lp_needs_precondition_for_the_pass(monkeypatch):
    _, prob = small_problem()
    no_device_work(monkeypatch)
    with pytest.raises(ValueError, match="precondition"):
        tp.solve_lp(prob, device="cpu", pock_chambolle=True)
    with pytest.raises(ValueError, match="precondition"):
        tp.solve_lp(prob, device="cpu", pock_chambolle=True, precondition=False, adaptive_stepsize=True)


def test_solve_lp_batch_needs_precondition_for_the_pass(monkeypatch):
    f, prob = small_problem()
    no_device_work(monkeypatch)
    with pytest.raises(ValueError, match="precondition"):
        tp.solve_lp_batch(prob, f.C, device="cpu", pock_chambolle=True)
    with pytest.raises(ValueError, match="precondition"):
        tp.solve_lp_batch(prob, f.C, device="cpu", pock_chambolle=True, K_values=f.val.view(-1, 1).repeat(1, 3))


def test_sharded_solves_refuse_the_pass(monkeypatch):
    _, prob = small_problem()
    for name in ("load_problem", "ruiz_precondition", "equilibrate_matrix", "ruiz_precondition_batch", "pdlp_algorithm",
                 "_solve_lp_sharded"):
        monkeypatch.setattr(tp.api, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("device work")))
    two_ranks = types.SimpleNamespace(world=2, rank=0)
    with pytest.raises(ValueError, match="pock_chambolle"):
        tp.solve_lp(prob, device="cpu", precondition=True, pock_chambolle=True, comm=two_ranks)
    # the batch refuses sharding as it did, with or without the pass
    f, _ = small_problem()
    monkeypatch.setattr(tp.batch, "BatchEngine", None)
    with pytest.raises(ValueError):
        tp.solve_lp_batch(prob, f.C, device="cpu", precondition=True, pock_chambolle=True, comm=two_ranks)


def test_k_values_with_the_pass_still_has_no_streamed_form(monkeypatch):
    f, prob = small_problem(B=16)
    no_device_work(monkeypatch)
    with pytest.raises(ValueError, match="streamed"):
        tp.solve_lp_batch(prob, f.C, device="cpu", precondition=True, pock_chambolle=True, slots=8,
                          K_values=f.val.view(-1, 1).repeat(1, 16))


def test_cli_takes_the_flag():
    from torchpdlp_amd.__main__ import parse_args
    assert parse_args(["--precondition", "--pock_chambolle"]).pock_chambolle is True
    assert parse_args(["--precondition"]).pock_chambolle is False


def test_the_functions_take_the_keyword():
    import inspect
    from torchpdlp_amd import precondition as pc
    for fn in (tp.solve_lp, tp.solve_lp_batch, pc.ruiz_precondition, pc.ruiz_precondition_batch):
        p = inspect.signature(fn).parameters["pock_chambolle"]
        assert p.default is False, fn.__name__
    assert list(inspect.signature(pc.pock_chambolle_pass).parameters)[:3] == ["lib", "code", "stream"]
    assert "pock_chambolle" not in inspect.signature(pc.ruiz_precondition_shard).parameters


def test_factor_entry_point_rejects_nonsense_without_a_gpu():
    lib = N.load()
    assert "pdlp_csr_row_l1_factors" in N.SIGNATURES and N.ABI_VERSION == 18 and lib.pdlp_abi_version() == 18
    assert lib.pdlp_csr_row_l1_factors(7, 1, None, None, None, None) == -1           # bad dtype code
    assert lib.pdlp_csr_row_l1_factors(N.PDLP_F32, -1, None, None, None, None) == -1
    assert lib.pdlp_csr_row_l1_factors(N.PDLP_F32, 4, None, None, None, None) == -1  # rows without a row pointer
    assert lib.pdlp_csr_row_l1_factors(N.PDLP_F64, 0, None, None, None, None) == 0   # no rows: nothing to launch
    with pytest.raises(N.PdlpError, match="no CPU fallback"):
        f, prob = small_problem()
        tp.ruiz_precondition(prob[0], prob[1], prob[2], prob[4], prob[5], device=torch.device("cpu"), pock_chambolle=True)
