"""CPU checks of ``precondition.Scaling`` -- the one place that scales vectors by the equilibration factors and un-scales iterates --
against the expressions written out, bit for bit, for every shape ``solve_lp``, ``solve_lp_batch`` and the sharded solve pass in;
and of the argument rules of ``equilibrate`` / ``equilibrate_matrix``, which hold before any device work."""
import itertools
import types

import pytest
import torch

import torchpdlp_amd as tp
from torchpdlp_amd import _native as N

n, m, B = 5, 3, 4
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
INF = float("inf")


def factors(dtype, per_lp):
    """``(D_col, D_row)``: 1-D (shared matrix) or ``(len, B)`` (a matrix per LP); entry 0 is exactly 1"""
    g = torch.Generator().manual_seed(3)
    draw = lambda ln: (10.0 ** (4 * torch.rand(ln, B, generator=g, dtype=torch.float64) - 2)).to(dtype)
    dc, dr = draw(n), draw(m)
    dc[0], dr[0] = 1.0, 1.0
    return (dc, dr) if per_lp else (dc[:, 0].clone(), dr[:, 0].clone())


def vector(ln, shape, dtype, seed, bound=None):
    """None, ``(ln,)``, ``(ln, 1)`` or ``(ln, B)``; ``bound``: entries 0 and 1 are -inf / +inf (entry 0 meets the factor 1)"""
    if shape is None:
        return None
    v = torch.randn(ln, B, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)
    if bound is not None:
        v[0], v[1] = -bound * INF, bound * INF
    return {"1d": v[:, 0].clone(), "col": v[:, :1].clone(), "wide": v}[shape]


def wide(t):
    """what ``api.py`` wrote out: a 1-D operand meets a 2-D one as a column"""
    return t if t.dim() == 2 else t.view(-1, 1)


def written_out(v, D, op):
    if v is None:
        return None
    if v.dim() == 1 and D.dim() == 1:
        return op(v, D)                       # a 1-D vector over a shared matrix stays 1-D
    return op(wide(v), wide(D))


SHAPES = [None, "1d", "col", "wide"]


@DTYPES
@pytest.mark.parametrize("per_lp", [False, True], ids=["shared", "per_lp"])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_scale_equals_the_written_out_expressions(dtype, per_lp, shape):
    dc, dr = factors(dtype, per_lp)
    sc = tp.Scaling(dc, dr)
    c, q = vector(n, shape, dtype, 1), vector(m, shape, dtype, 2)
    l, u = vector(n, shape, dtype, 3, bound=1), vector(n, shape, dtype, 4, bound=-1)     # l: -inf, +inf; u: +inf, -inf
    kept = [None if v is None else v.clone() for v in (c, q, l, u, dc, dr)]
    got = sc.scale(c, q, l, u)
    want = (written_out(c, dc, torch.mul), written_out(q, dr, torch.mul), written_out(l, dc, torch.div), written_out(u, dc, torch.div))
    for name, g, w, v in zip("cqlu", got, want, (c, q, l, u)):
        if shape is None:
            assert g is None, name
            continue
        assert g.dtype == dtype and g.shape == w.shape and torch.equal(g, w), name
        assert not torch.isnan(g).any(), name
        assert g.data_ptr() != v.data_ptr(), name                      # a new tensor
        rows = v.shape[0]
        expect = (rows,) if shape == "1d" and not per_lp else (rows, B if per_lp or shape == "wide" else 1)
        assert tuple(g.shape) == expect, (name, tuple(g.shape), expect)
    if shape is not None:                          # infinite bounds keep their sign, also where the factor is exactly 1
        for g, v in ((got[2], l), (got[3], u)):
            inf_in = torch.isinf(wide(v)).expand_as(wide(g))
            assert torch.equal(torch.isinf(wide(g)), inf_in)
            assert torch.equal(torch.sign(wide(g))[inf_in], torch.sign(wide(v)).expand_as(wide(g))[inf_in])
        assert torch.equal(wide(got[0])[0], wide(c)[0].expand_as(wide(got[0])[0]))           # the factor 1: c itself
    for a, b in zip(kept, (c, q, l, u, dc, dr)):   # the inputs are as they were
        assert a is None or torch.equal(a, b)


@DTYPES
@pytest.mark.parametrize("per_lp", [False, True], ids=["shared", "per_lp"])
@pytest.mark.parametrize("shape", SHAPES[1:])
def test_unscale_equals_the_written_out_products(dtype, per_lp, shape):
    """the factors are cast to the iterate's dtype first (a float32 iterate under float64 factors and the other way round)"""
    for fdt in (torch.float32, torch.float64):
        dc, dr = factors(fdt, per_lp)
        sc = tp.Scaling(dc, dr)
        x, y = vector(n, shape, dtype, 5), vector(m, shape, dtype, 6)
        kept = [t.clone() for t in (x, y, dc, dr)]
        gx, gy = sc.unscale_x(x), sc.unscale_y(y)
        wx, wy = written_out(x, dc.to(dtype), lambda v, D: D * v), written_out(y, dr.to(dtype), lambda v, D: D * v)
        assert gx.dtype == dtype and gx.shape == wx.shape and torch.equal(gx, wx)
        assert gy.dtype == dtype and gy.shape == wy.shape and torch.equal(gy, wy)
        for a, b in zip(kept, (x, y, dc, dr)):
            assert torch.equal(a, b)


def test_the_written_out_expressions_are_those_of_the_front_ends():
    """``written_out`` against the three forms the package had: ``solve_lp`` (``(n, 1)`` factors and iterate), the batch over a shared
    matrix (``sc``: a 1-D vector through a column and back) and the batch with a matrix per LP (``wide``)"""
    dt = torch.float32
    dc, _ = factors(dt, False)
    dcB, _ = factors(dt, True)
    v1, vB = vector(n, "1d", dt, 7), vector(n, "wide", dt, 7)
    sc_ = lambda v, D, op: (op(v.view(-1, 1), D).view(-1) if v.dim() == 1 else op(v, D.to(v.device)))
    for op in (torch.mul, torch.div):
        assert torch.equal(written_out(v1, dc, op), sc_(v1, dc.view(-1, 1), op))
        assert torch.equal(written_out(vB, dc, op), sc_(vB, dc.view(-1, 1), op))
        assert torch.equal(written_out(v1, dcB, op), op(v1.view(-1, 1), dcB))
        assert torch.equal(written_out(vB, dcB, op), op(vB, dcB))
    x = vector(n, "col", dt, 8)
    assert torch.equal(tp.Scaling(dc.view(-1, 1), dc.view(-1, 1)).unscale_x(x), dc.view(-1, 1).to(x.dtype) * x)      # solve_lp
    X = vector(n, "wide", dt, 8)
    for d in (dc.view(-1, 1), dcB):                                                                                    # solve_lp_batch
        assert torch.equal(tp.Scaling(d, d).unscale_x(X), d.reshape(d.shape[0], -1).to(X.dtype) * X)


def small_matrix():
    f = tp.gen_lp_family(30, 20, 3, 1, seed=1)
    return tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val)


def test_equilibration_has_no_cpu_fallback():
    K = small_matrix()
    before = K.val.clone()
    for flag in (False, True):
        with pytest.raises(N.PdlpError, match="no CPU fallback"):
            tp.equilibrate_matrix(K, device=torch.device("cpu"), pock_chambolle=flag)
        with pytest.raises(N.PdlpError, match="no CPU fallback"):
            tp.equilibrate((K.rowptr, K.colidx, K.val), (K.t_rowptr, K.t_colidx, K.t_val), pock_chambolle=flag)
    assert torch.equal(K.val, before)


def test_equilibrate_refuses_the_sharded_pass_before_any_device_work(monkeypatch):
    K = small_matrix()
    monkeypatch.setattr(N, "load", lambda: (_ for _ in ()).throw(AssertionError("device work before the argument checks")))
    two_ranks = types.SimpleNamespace(world=2, rank=0)
    with pytest.raises(ValueError, match="pock_chambolle"):
        tp.equilibrate((K.rowptr, K.colidx, K.val), (K.t_rowptr, K.t_colidx, K.t_val), comm=two_ranks, pock_chambolle=True)
    # a communicator of one rank is the single-process case: the pass is allowed, and the CPU matrix is what is refused
    with pytest.raises(N.PdlpError, match="no CPU fallback"):
        tp.equilibrate((K.rowptr, K.colidx, K.val), (K.t_rowptr, K.t_colidx, K.t_val), comm=types.SimpleNamespace(world=1, rank=0),
                       pock_chambolle=True)


def test_the_new_functions_keep_the_issue_signatures():
    import inspect
    from torchpdlp_amd import precondition as pc
    assert list(inspect.signature(pc.equilibrate).parameters) == ["K_blk", "KT_blk", "comm", "r0", "c0", "max_iter", "eps", "pock_chambolle"]
    assert list(inspect.signature(pc.equilibrate_matrix).parameters) == ["K", "device", "max_iter", "eps", "pock_chambolle"]
    assert [f.name for f in pc.Scaling.__dataclass_fields__.values()] == ["d_col", "d_row", "sweeps", "seconds"]
    assert list(itertools.islice(inspect.signature(pc._sweeps).parameters, 3)) == ["lib", "code", "stream"]
