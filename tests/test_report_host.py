"""The solution report (duals, reduced costs, row activities, residuals) as far as it can be checked without a GPU: the result
types, the binding against the header, and the argument checks of the two entry points."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import torch

import torchpdlp_amd as tp
from torchpdlp_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_FIELDS = ("y", "reduced_costs", "row_activity", "dual_objective", "primal_residual", "dual_residual", "gap",
                 "rel_primal_residual", "rel_dual_residual", "rel_gap")


def test_lpresult_keeps_its_seven_positional_fields_and_tuple():
    x = torch.zeros(3, 1)
    r = tp.LPResult(x, 1.5, 10, 2, 14, "Solved", 0.25)
    assert r.as_tuple() == (x, 1.5, 10, 2, 14, "Solved", 0.25) and len(r.as_tuple()) == 7
    names = [f.name for f in dataclasses.fields(tp.LPResult)]
    assert names[:7] == ["x", "objective", "iterations", "restarts", "kkt_passes", "status", "time"]
    assert tuple(names[7:]) == REPORT_FIELDS
    assert all(getattr(r, name) is None for name in REPORT_FIELDS)


def test_batchresult_has_the_report_fields_and_passes_them_on():
    X, Y = torch.arange(6.0).view(3, 2), torch.arange(4.0).view(2, 2)
    one = lambda v: np.asarray(v)
    plain = tp.BatchResult(X, Y, one([1.0, 2.0]), one([3, 4]), one([1, 1]), one([5, 6]), ["Solved", "Solved"], 0.5)
    assert all(getattr(plain, name) is None for name in REPORT_FIELDS[1:])
    assert plain[1].y is None and plain[1].reduced_costs is None and len(plain[1].as_tuple()) == 7
    rep = dict(y=Y, reduced_costs=X + 10, row_activity=Y + 20, pr=one([1.0, 2.0]), dr=one([3.0, 4.0]), gap=one([-0.5, 0.25]),
               p=one([1.0, -3.0]), d_adj=one([0.5, -2.75]), q_norm=one([1.0, 3.0]), c_norm=one([0.0, 1.0]))
    f = tp.report_fields(rep)
    f.pop("y")
    full = tp.BatchResult(X, Y, one([1.0, -3.0]), one([3, 4]), one([1, 1]), one([5, 6]), ["Solved", "Solved"], 0.5, **f)
    r = full[1]
    assert torch.equal(r.y, Y[:, 1:2]) and torch.equal(r.reduced_costs, X[:, 1:2] + 10) and torch.equal(r.row_activity, Y[:, 1:2] + 20)
    assert r.dual_objective == -2.75 and r.primal_residual == 2.0 and r.dual_residual == 4.0 and r.gap == 0.25
    assert r.rel_primal_residual == 2.0 / 4.0 and r.rel_dual_residual == 4.0 / 2.0 and r.rel_gap == 0.25 / (1 + 3.0 + 2.75)


def test_report_fields_are_the_left_hand_sides_of_check_termination():
    rep = dict(y=None, reduced_costs=None, row_activity=None, pr=3e-4, dr=2e-4, gap=-1e-3, p=10.0, d_adj=9.999, q_norm=2.0, c_norm=4.0)
    f = tp.report_fields(rep)
    for tol in (1e-3, 1e-4, 5e-5, 1e-5):
        want = tp.check_termination(rep["pr"], rep["dr"], rep["gap"], rep["p"], rep["d_adj"], 2.0, 4.0, tol)
        got = f["rel_primal_residual"] <= tol and f["rel_dual_residual"] <= tol and f["rel_gap"] <= tol
        assert bool(want) == bool(got)
    assert tp.report_fields(None) == {} and f["gap"] == -1e-3 and f["dual_objective"] == 9.999


def test_binding_and_header_declare_the_report_entry_points():
    src = open(os.path.join(ROOT, "include", "pdlp_hip.h")).read()
    for name, nargs in (("pdlp_report_local", 5), ("pdlp_batch_report", 7)):
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == nargs
        decl = re.search(r"int %s\((.*?)\);" % name, src, flags=re.S)
        assert decl is not None and len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == nargs
    assert N.ABI_VERSION == 18 and N.load().pdlp_abi_version() == 18
    body = re.search(r"typedef struct pdlp_batch \{(.*?)\} pdlp_batch;", src, flags=re.S).group(1)
    assert "rc" not in re.findall(r"(\w+);", body) and len(N.PdlpBatch._fields_) == 31       # the new buffers are arguments


def test_report_entry_points_reject_nonsense_without_a_gpu():
    lib = N.load()
    b = N.PdlpBatch()
    assert lib.pdlp_report_local(None, 0, 0, None, None) == -1
    assert lib.pdlp_report_local(None, 5, 0, None, None) == -1
    assert lib.pdlp_batch_report(None, C.byref(b), 0, 0, 0, None, None) == -1
    assert lib.pdlp_batch_report(None, None, 0, 0, 0, None, None) == -1
    assert lib.pdlp_batch_report(None, C.byref(b), 5, 0, 0, None, None) == -1
    assert lib.pdlp_batch_report(None, C.byref(b), 0, 0, 3, None, None) == -1


def test_solution_file_of_the_cli_holds_the_result(tmp_path):
    from torchpdlp_amd.__main__ import SOLUTION_SCALARS, parse_args, write_solution
    assert parse_args([]).solution_dir is None and parse_args(["--solution_dir", "s"]).solution_dir == "s"
    v = lambda ln, a: torch.arange(ln, dtype=torch.float32).view(-1, 1) + a
    r = tp.LPResult(v(3, 0), 1.5, 10, 2, 14, "Solved", 0.25, y=v(2, 1), reduced_costs=v(3, 2), row_activity=v(2, 3), dual_objective=1.25,
                    primal_residual=1e-3, dual_residual=2e-3, gap=-0.25, rel_primal_residual=1e-4, rel_dual_residual=2e-4, rel_gap=-0.1)
    z = np.load(write_solution(str(tmp_path / "sol"), "afiro.mps", r))
    assert os.path.basename(write_solution(str(tmp_path / "sol"), "afiro.mps", r)) == "afiro.npz"
    for k in ("x", "y", "reduced_costs", "row_activity"):
        np.testing.assert_array_equal(z[k], getattr(r, k).numpy().reshape(-1))
    for k in SOLUTION_SCALARS:
        assert z[k] == getattr(r, k)
    assert str(z["status"]) == "Solved"
