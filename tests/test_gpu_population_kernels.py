"""The population kernels (pdlp_kernel_mv.inc, pdlp_population.inc: ``mv_steps``, ``mv_gap``, ``mv_product``, ``mv_combine``) one
call at a time against the float64 model of ``tests/population_model.py`` (pinned by ``tests/test_population_model_host.py``), on
ALL j columns, at 8, 16 and 32 points, in float32 and float64.

Every comparison is bit for bit or ``C_BOUND`` times the model's running-error bound of the kernel's own arithmetic (the rules at the
top of ``tests/test_gpu_batch_kernels.py``); ``judge`` prints the largest ``error / bound`` of each comparison.  X, Y and every
output are views inside larger buffers of the suite's signalling-NaN pattern, ``GUARD`` rows before and after: after every call the
guards hold the same bytes and every output entry is finite.  The work buffers hold the same pattern before each call, so nothing
is read before it is written.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import torchpdlp_amd as tp
from torchpdlp_amd import _native as N
from tests import population_model as pm
from tests import test_gpu_batch_kernels as bk

pytestmark = pytest.mark.gpu

C_BOUND, TORCH, IVIEW, dev, units = bk.C_BOUND, bk.TORCH, bk.IVIEW, bk.dev, bk.units
GUARD = 64
WIDTHS = (8, 16, 32)
CASES = ["1x1", "ineq0", "ineq_all", "empty_rows_cols", "long_row", "odd_rows", "mixed_400x300"]
OMEGA = 1.3
TYPES = pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
WIDTH = pytest.mark.parametrize("j", WIDTHS)


# ---------------------------------------------------------------------------------------------------------------------------------
# LPs, engines, guarded buffers
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lp_of(case, T):
    rng = np.random.default_rng(CASES.index(case) if case in CASES else 99)
    if case == "mixed_400x300":
        return bk.golden_lp(T, 1, rng, per="cqlu")[0]
    if case == "big":                 # m = 300 000, n = 70 000
        return bk.big_lp(T, 1, rng)
    if case == "wide":
        return bk.big_lp(T, 1, rng, m=70_000, n=300_000)
    return bk.shape_lp(case, T, 1, "cqlu", rng)


def make_engine(P, vec_dtype=None):
    K = P.csr()
    T = P.T if vec_dtype is None else np.float64
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v.astype(T))).to(dev())
    return tp.PdlpEngine(P.m, P.n, P.m_ineq, (K.rowptr, K.colidx, K.val), (K.t_rowptr, K.t_colidx, K.t_val), *(d(v) for v in P.col(0)),
                         vec_dtype=vec_dtype, tiles=False)


@functools.lru_cache(maxsize=None)
def engine_of(case, T):
    return make_engine(lp_of(case, T))


class Pop:
    """[rows, j] of T as a view inside a [rows + 2 GUARD, j] buffer of the poison pattern; the view holds ``values`` if given"""

    def __init__(self, rows, j, T, values=None):
        host = bk.poison((rows + 2 * GUARD, j), T)
        if values is not None:
            host[GUARD:GUARD + rows] = values
        self.rows, self.T = rows, T
        self.buf = torch.from_numpy(host).to(dev())
        self.v = self.buf[GUARD:GUARD + rows]
        assert self.v.is_contiguous() and self.v.shape == (rows, j)

    def guards_intact(self, what):
        bits = bk.POISON[self.T][1]
        iv = self.buf.view(IVIEW[self.buf.dtype])
        ok = bool((iv[:GUARD] == bits).all()) and bool((iv[GUARD + self.rows:] == bits).all())
        assert ok, f"{what}: a guard row was written"

    def get(self, what):
        """the view as float64, every entry finite"""
        a = self.v.double().cpu().numpy()
        assert np.isfinite(a).all(), f"{what}: an output entry is not finite"
        return a

    def bits(self):
        return self.v.contiguous().view(IVIEW[self.v.dtype]).cpu().numpy().copy()


def sync():
    torch.cuda.synchronize()


def mv_steps(eng, X, Y, k, eta, omega=OMEGA, theta=1.0):
    """``eng.mv_steps`` on the views of X and Y with the work buffer poisoned and guarded"""
    j = X.v.shape[1]
    work = Pop(2 * eng.n + eng.m, j, X.T)
    eng._mv_work[j] = work.v.view(-1)
    eng.mv_steps(X.v, Y.v, k, eta, omega, theta)
    sync()
    for b, nm in ((X, "X"), (Y, "Y"), (work, "work")):
        b.guards_intact(f"mv_steps({k}) {nm}")
    return X.get(f"mv_steps({k}) X"), Y.get(f"mv_steps({k}) Y")


def mv_product(eng, X):
    """``pdlp_mv_product`` into a guarded output; ``eng.mv_product`` gives the same bits"""
    j = X.v.shape[1]
    out = Pop(eng.m, j, X.T)
    eng._mv_check(X.v, out.v)
    N.check(eng.lib.pdlp_mv_product(eng.h, j, X.v.data_ptr(), out.v.data_ptr()), "pdlp_mv_product")
    own = eng.mv_product(X.v)
    sync()
    X.guards_intact("mv_product X")
    out.guards_intact("mv_product out")
    val = out.get("mv_product")
    assert np.array_equal(out.bits(), own.view(IVIEW[own.dtype]).cpu().numpy())
    return val, out


def mv_gap(eng, X, Y):
    """``pdlp_mv_gap`` with its work buffer poisoned and guarded; ``eng.mv_gap`` gives the same bits"""
    j = X.v.shape[1]
    eng._mv_check(X.v, Y.v)
    work = Pop(256 * 4 + 4, j, np.float64)                 # (engine.mv_gap's size: 256 * j * 4 + j * 4 doubles)
    out = (C.c_double * j)()
    N.check(eng.lib.pdlp_mv_gap(eng.h, j, X.v.data_ptr(), Y.v.data_ptr(), work.v.data_ptr(), out), "pdlp_mv_gap")
    own = eng.mv_gap(X.v, Y.v)
    sync()
    for b, nm in ((X, "X"), (Y, "Y"), (work, "work")):
        b.guards_intact(f"mv_gap {nm}")
    g = np.array(list(out))
    assert np.isfinite(g).all(), "mv_gap: a gap is not finite"
    assert g.tobytes() == np.array(own).tobytes()
    return g


def judge(kernel, T, what, got, ref, err):
    """bk.close, all entries, after printing the largest error / bound"""
    got, ref, err = (np.asarray(v, np.float64) for v in (got, ref, err))
    assert got.shape == ref.shape == err.shape, (what, got.shape, ref.shape, err.shape)
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, d / err, np.where(d > 0, np.inf, 0.0))
    print(f"error/bound {kernel} {T.__name__} {float(ratio.max()) if ratio.size else 0.0:.4f} ({what})")
    bk.close(what, got, ref, err)


def one_step_product_gap(case, T, j, X0, Y0, what):
    """one mv_steps(1), one mv_product and one mv_gap on all j columns against the model"""
    P, eng, u = lp_of(case, T), engine_of(case, T), units(T)
    eta = bk.eta_base(P)
    X, Y = Pop(P.n, j, T, X0), Pop(P.m, j, T, Y0)
    kx, _ = mv_product(eng, X)
    rk, ek = pm.product(P, X0, u)
    judge("mv_product", T, f"{what} product", kx, rk, ek)
    x1, y1 = mv_steps(eng, X, Y, 1, eta)
    rx, ry, ex, ey = pm.steps(P, X0, Y0, 1, eta, OMEGA, 1.0, T, u)
    judge("mv_steps", T, f"{what} X after one step", x1, rx, ex)
    judge("mv_steps", T, f"{what} Y after one step", y1, ry, ey)
    gaps = mv_gap(eng, X, Y)
    rg, eg = pm.gap(P, x1, y1, T, u)                      # the model at the point the device holds
    judge("mv_gap", T, f"{what} gap", gaps, rg, eg)
    return rx, ry


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. one call of each entry point, every shape
# ---------------------------------------------------------------------------------------------------------------------------------
@TYPES
@WIDTH
@pytest.mark.parametrize("case", CASES)
def test_steps_one_call(case, j, T):
    P = lp_of(case, T)
    X0, Y0 = pm.draw_population(P, j, np.random.default_rng(1000 + j))
    rx, ry = one_step_product_gap(case, T, j, X0, Y0, f"{case} j={j}")
    if case != "1x1":                                      # the inputs do what they are drawn for
        _, _, l, hi = P.col(0)
        assert ((X0[:, 1::2] < l[:, None]) | (X0[:, 1::2] > hi[:, None])).any() and not (X0[:, 0::2] < l[:, None]).any()
        assert P.m_ineq == 0 or ((ry[:P.m_ineq] == 0).any() and (ry[:P.m_ineq] > 0).any())


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the buffers of mv_steps_n
# ---------------------------------------------------------------------------------------------------------------------------------
@TYPES
@WIDTH
@pytest.mark.parametrize("case", ["odd_rows", "mixed_400x300"])
def test_steps_buffers(case, j, T):
    P, eng, u = lp_of(case, T), engine_of(case, T), units(T)
    eta, theta = bk.eta_base(P), 0.75
    X0, Y0 = pm.draw_population(P, j, np.random.default_rng(2000 + j))
    X, Y = Pop(P.n, j, T, X0), Pop(P.m, j, T, Y0)
    bx, by = X.bits(), Y.bits()
    mv_steps(eng, X, Y, 0, eta, theta=theta)
    assert np.array_equal(X.bits(), bx) and np.array_equal(Y.bits(), by), "steps=0 wrote X or Y"
    one = {}
    X, Y = Pop(P.n, j, T, X0), Pop(P.m, j, T, Y0)
    for k in range(1, 7):                                  # k calls with steps=1
        mv_steps(eng, X, Y, 1, eta, theta=theta)
        one[k] = (X.bits(), Y.bits())
    for k in (2, 3, 6):                                    # the same kernels in the same order: no tolerance
        X, Y = Pop(P.n, j, T, X0), Pop(P.m, j, T, Y0)
        xk, yk = mv_steps(eng, X, Y, k, eta, theta=theta)
        assert np.array_equal(X.bits(), one[k][0]), f"steps={k}: X is not what {k} calls with steps=1 give"
        assert np.array_equal(Y.bits(), one[k][1]), f"steps={k}: Y is not what {k} calls with steps=1 give"
        if k == 3:
            rx, ry, ex, ey = pm.steps(P, X0, Y0, 3, eta, OMEGA, theta, T, u)
            judge("mv_steps", T, f"{case} j={j} X after three steps", xk, rx, ex)
            judge("mv_steps", T, f"{case} j={j} Y after three steps", yk, ry, ey)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. a column's result depends on nothing but that column
# ---------------------------------------------------------------------------------------------------------------------------------
def run_all(case, T, X0, Y0, k):
    """k steps (one call), the product of X0, the gap after the steps -> bits of X, Y, K X0; gaps; the stepped point"""
    P, eng = lp_of(case, T), engine_of(case, T)
    j = X0.shape[1]
    X, Y = Pop(P.n, j, T, X0), Pop(P.m, j, T, Y0)
    _, out = mv_product(eng, X)
    xk, yk = mv_steps(eng, X, Y, k, bk.eta_base(P))
    return X.bits(), Y.bits(), out.bits(), mv_gap(eng, X, Y), xk, yk


@TYPES
@pytest.mark.parametrize("case", ["odd_rows", "mixed_400x300"])
def test_columns_are_independent(case, T):
    P, u = lp_of(case, T), units(T)
    rng = np.random.default_rng(3000)
    pops = {j: pm.draw_population(P, j, rng) for j in WIDTHS}
    # permuted columns: permuted outputs, bit for bit
    for j in WIDTHS:
        X0, Y0 = pops[j]
        perm = rng.permutation(j)
        assert (perm != np.arange(j)).any()
        a = run_all(case, T, X0, Y0, 3)
        b = run_all(case, T, X0[:, perm], Y0[:, perm], 3)
        for nm, va, vb in zip(("X", "Y", "K X"), a[:3], b[:3]):
            assert np.array_equal(va[:, perm], vb), f"j={j}: {nm} of the permuted population is not the permuted {nm}"
        rg, eg = pm.gap(P, a[4], a[5], T, u)
        judge("mv_gap", T, f"{case} j={j} gap", a[3], rg, eg)
        judge("mv_gap", T, f"{case} j={j} gap, permuted", b[3], rg[perm], eg[perm])
    # a point of the 8-wide population in another column of a 16-wide and of a 32-wide one: each lane walks its row in CSR order
    # whatever the width, so X, Y and K X agree bit for bit; the gap's partial sums are grouped otherwise: within the bound
    X8, Y8 = pops[8]
    a = run_all(case, T, X8, Y8, 3)
    rg, eg = pm.gap(P, a[4], a[5], T, u)
    src = [0, 3, 7]
    for j, dst in ((16, [15, 0, 6]), (32, [31, 0, 17])):
        X0, Y0 = (v.copy() for v in pops[j])
        X0[:, dst], Y0[:, dst] = X8[:, src], Y8[:, src]
        b = run_all(case, T, X0, Y0, 3)
        for nm, va, vb in zip(("X", "Y", "K X"), a[:3], b[:3]):
            assert np.array_equal(va[:, src], vb[:, dst]), f"{nm}: columns {src} at width 8 differ from columns {dst} at width {j}"
        judge("mv_gap", T, f"{case} gap at width {j} against width 8", b[3][dst], a[3][src], eg[src])
        judge("mv_gap", T, f"{case} gap at width {j}", b[3][dst], rg[src], eg[src])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. every grid-stride loop takes a second pass
# ---------------------------------------------------------------------------------------------------------------------------------
MV_MAX_GRID, MV_GAP_GRID, WAVES = 8192, 256, 4            # mv_grid's cap, mv_gap_n's cap, waves per workgroup (BLOCK / 64)


def mv_grid(rows, j, cap=MV_MAX_GRID):
    per_block = (64 // j) * WAVES
    return min(max(-(-rows // per_block), 1), cap)


def passes(rows, j, cap=MV_MAX_GRID):
    """iterations of the ``r0 += nwaves * RPW`` loop of the wave that takes the most"""
    return -(-rows // (mv_grid(rows, j, cap) * WAVES * (64 // j)))


@functools.lru_cache(maxsize=None)
def big_population(case, T):
    P = lp_of(case, T)
    return pm.draw_population(P, 32, np.random.default_rng(4000))


@pytest.mark.parametrize("case,T", [("big", np.float32), ("big", np.float64), ("wide", np.float32)], ids=["big-f32", "big-f64", "wide-f32"])
@WIDTH
def test_grid_stride(case, T, j):
    P = lp_of(case, T)
    if case == "big":
        assert passes(P.m, j) >= 2, "DualMV / StoreMV over K must stride"
        assert j != 32 or passes(P.n, j) >= 2, "PrimalMV over K' must stride at 32 points"
    else:
        assert passes(P.n, j) >= 2 or j == 32, "PrimalMV over K' must stride at 8 and 16 points"
    assert passes(P.n, j, MV_GAP_GRID) >= 2 and passes(P.m, j, MV_GAP_GRID) >= 2, "GapMV and k_mv_dot must stride"
    assert mv_grid(P.n, j, MV_GAP_GRID) == mv_grid(P.m, j, MV_GAP_GRID) == MV_GAP_GRID, "k_mv_finalize must add every block"
    X0, Y0 = big_population(case, T)
    one_step_product_gap(case, T, j, X0[:, :j], Y0[:, :j], f"{case} j={j}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. mv_combine
# ---------------------------------------------------------------------------------------------------------------------------------
def weights(kind, j, nw, T, rng):
    """columns of convex weights as fishnet makes them (w / w.sum()); one column all zero; entries of both signs"""
    W = rng.uniform(0, 1, (j, nw)).astype(T)
    W = (W / W.sum(0)).astype(T)
    if kind == "zero_column":
        W[:, nw // 2] = 0
    elif kind == "negative":
        W = (W * rng.choice([-1.0, 1.0], (j, nw)) * 3).astype(T)
    return W


def mv_combine(eng, V0, W0, T):
    """``pdlp_mv_combine`` from a guarded V into a guarded output; ``eng.mv_combine`` gives the same bits"""
    rows, j = V0.shape
    nw = W0.shape[1]
    V, Wd, out = Pop(rows, j, T, V0), Pop(j, nw, T, W0), Pop(rows, nw, T)
    N.check(eng.lib.pdlp_mv_combine(N.PDLP_F32 if T == np.float32 else N.PDLP_F64, rows, j, V.v.data_ptr(), Wd.v.data_ptr(), nw,
                                     out.v.data_ptr(), eng.stream.cuda_stream), "pdlp_mv_combine")
    own = eng.mv_combine(V.v, Wd.v)
    sync()
    for b, nm in ((V, "V"), (Wd, "W"), (out, "out")):
        b.guards_intact(f"mv_combine {nm}")
    val = out.get("mv_combine")
    assert own.shape == (rows, nw) and np.array_equal(out.bits(), own.view(IVIEW[own.dtype]).cpu().numpy())
    return val


COMBINE_J, COMBINE_NW = (1, 2, 7, 31, 32), (1, 5, 31, 32)


@TYPES
@pytest.mark.parametrize("rows", [1, 63, 257, 70_000])
def test_combine(rows, T):
    eng, u = engine_of("1x1", T), units(T)
    rng = np.random.default_rng(rows)
    shapes = [(j, nw) for j in COMBINE_J for nw in COMBINE_NW] if rows < 70_000 else [(32, 32), (31, 8), (8, 31)]
    if rows == 70_000:                                     # past the grid-stride loop's first pass: MAX_GRID workgroups of 256
        assert all(rows * nw > 524_288 for _, nw in shapes)
    for j, nw in shapes:
        V0 = rng.uniform(-2, 2, (rows, j)).astype(T)
        for kind in ("convex", "zero_column", "negative"):
            W0 = weights(kind, j, nw, T, rng)
            got = mv_combine(eng, V0, W0, T)
            ref, err = pm.combine(V0, W0, u)
            judge("mv_combine", T, f"combine rows={rows} j={j} nw={nw} {kind}", got, ref, err)
            if kind == "zero_column":
                assert not got[:, nw // 2].any()


@TYPES
def test_combine_refuses_0_and_33(T):
    eng = engine_of("1x1", T)
    t = lambda *shape: torch.ones(*shape, dtype=TORCH[T], device=dev())
    for j, nw in ((0, 3), (33, 3), (3, 0), (3, 33)):
        with pytest.raises(ValueError):
            eng.mv_combine(t(5, j), t(j, nw))
    with pytest.raises(ValueError):                        # W of another j
        eng.mv_combine(t(5, 4), t(3, 2))
    with pytest.raises(ValueError):                        # V of another precision
        eng.mv_combine(torch.ones(5, 4, dtype=TORCH[np.float64 if T == np.float32 else np.float32], device=dev()), t(4, 2))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. refusals leave X and Y as they were
# ---------------------------------------------------------------------------------------------------------------------------------
def calls(eng, Xv, Yv):
    return (("mv_steps", lambda: eng.mv_steps(Xv, Yv, 1, 0.1, OMEGA)), ("mv_gap", lambda: eng.mv_gap(Xv, Yv)),
            ("mv_product", lambda: eng.mv_product(Xv)))


@TYPES
def test_refusals(T):
    case = "odd_rows"
    P, eng = lp_of(case, T), engine_of(case, T)
    other = np.float64 if T == np.float32 else np.float32
    rng = np.random.default_rng(6000)

    def refused(what, error, Xp, Yp, Xv, Yv, e=eng, only=None, **kw):
        bx, by = Xp.buf.view(IVIEW[Xp.buf.dtype]).clone(), Yp.buf.view(IVIEW[Yp.buf.dtype]).clone()
        for nm, call in calls(e, Xv, Yv):
            if only is None or nm in only:
                with pytest.raises(error, **kw):
                    call()
        sync()
        assert torch.equal(Xp.buf.view(IVIEW[Xp.buf.dtype]), bx) and torch.equal(Yp.buf.view(IVIEW[Yp.buf.dtype]), by), f"{what}: X or Y was written"

    def pops(j, T=T, n=P.n, m=P.m):
        return Pop(n, j, T, rng.uniform(-1, 1, (n, j))), Pop(m, j, T, rng.uniform(-1, 1, (m, j)))

    for j in (1, 4, 7, 12, 24, 33, 64):                    # widths other than 8, 16, 32
        X, Y = pops(j)
        refused(f"width {j}", ValueError, X, Y, X.v, Y.v)
    X, Y = pops(8, n=P.n + 1)                              # wrong shapes
    refused("n + 1 rows of X", ValueError, X, Y, X.v, Y.v)
    X, Y = pops(8, m=P.m - 1)
    refused("m - 1 rows of Y", ValueError, X, Y, X.v, Y.v, only=("mv_steps", "mv_gap"))
    X, _ = pops(8)
    _, Y = pops(16)
    refused("X of 8 and Y of 16 columns", ValueError, X, Y, X.v, Y.v, only=("mv_steps", "mv_gap"))
    X, Y = pops(8)
    refused("1-D X", ValueError, X, Y, X.v.reshape(-1), Y.v)
    X, Y = pops(16)                                        # not contiguous
    refused("every second column", ValueError, X, Y, X.v[:, ::2], Y.v[:, ::2])
    X, Y = pops(P.n, n=8), pops(P.m, m=8)[1]               # [8, n] and [8, m]: their transposes have the right shape
    refused("transposed views", ValueError, X[0], Y, X[0].v.t(), Y.v.t())
    X, Y = pops(8, T=other)                                # the wrong precision
    refused("the other precision", ValueError, X, Y, X.v, Y.v)
    if T == np.float64:                                    # float32 matrix under float64 vectors: the library refuses (PDLP_ERR_STATE)
        mixed = make_engine(lp_of(case, np.float32), vec_dtype=torch.float64)
        assert mixed.mixed
        X, Y = pops(8)
        refused("a mixed-precision engine", N.PdlpError, X, Y, X.v, Y.v, e=mixed, match=r"call sequence.*\(code -3\)")
