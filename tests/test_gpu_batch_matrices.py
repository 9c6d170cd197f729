"""Batched solves with a constraint matrix per LP over one shared pattern (``K_values``, pdlp_batch_attach_matrices) on the MI355X.

Bit-identity: the per-LP row walk keeps the summation order of the shared-matrix one, so (1) a batch whose ``K_values`` columns all
equal ``K.val`` returns the bits of the batch without ``K_values``, and (2) LP b of a batch with genuinely different matrices
returns the bits of a shared-matrix batch of that one LP over matrix b at the same W.  Accuracy: every entry point call by call
against the float64 references of tests/test_gpu_batch_kernels.py and tests/test_gpu_report.py (their helpers, their bounds), LP by
LP over that LP's matrix; the plain product, the per-LP power iteration and the per-LP Ruiz factors.  End to end: a
``matrix_noise`` family against its built-in optima, against ``solve_lp`` per LP and against HiGHS.
"""
import os
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import torchpdlp_amd as tp
from torchpdlp_amd import _native as N
from torchpdlp_amd.batch import BatchEngine, estimate_sigma_batch, pdlp_algorithm_batch
from torchpdlp_amd.precondition import equilibrate_matrix, ruiz_precondition_batch
from tests import test_gpu_batch_kernels as bk
from tests import test_gpu_report as rp_

pytestmark = pytest.mark.gpu

TORCH = bk.TORCH
IVIEW = bk.IVIEW


def dev():
    return torch.device("cuda", 0)


def family(B, seed, noise=0.2, n=300, m=240, dtype=torch.float32):
    return tp.gen_lp_family(n, m, 4, B, seed=seed, dtype=dtype, matrix_noise=noise)


def csr(f, vals=None):
    K = tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val)
    return (K if vals is None else K.with_values(vals.contiguous())).to(dev())


def dense(f, vals):
    """LP b's matrix as a float64 array (a column held twice in a row is summed, as the kernels add both items)"""
    v = np.ascontiguousarray(vals.double().cpu().numpy())
    return sp.csr_matrix((v, f.colidx.numpy().copy(), f.rowptr.numpy().copy()), shape=(f.m, f.n)).toarray()


def norm2(f, vals):
    return float(np.linalg.norm(dense(f, vals), 2))


def same_bits(a, b):
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(IVIEW[a.dtype]), b.contiguous().view(IVIEW[b.dtype]))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_solve(a, ra, b, rb, cols_a=None, cols_b=None, what=""):
    """x, y, the objective, k, n, j, the status and every report field of the chosen columns: the same bits"""
    pick = lambda v, cols: v if cols is None else (v[..., cols] if not isinstance(v, list) else [v[i] for i in cols])
    for i, nm in enumerate(("x", "y", "objective", "k", "n", "j")):
        assert same_bits(pick(a[i], cols_a), pick(b[i], cols_b)), f"{what}: {nm}"
    assert pick(a[6], cols_a) == pick(b[6], cols_b), f"{what}: status"
    assert set(ra) == set(rb) and {"y", "reduced_costs", "row_activity", "pr", "dr", "gap", "p", "d_adj", "kkt", "q_norm", "c_norm"} <= set(ra)
    for key in ra:
        assert same_bits(pick(ra[key], cols_a), pick(rb[key], cols_b)), f"{what}: report field {key}"


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. bit-identity
# ---------------------------------------------------------------------------------------------------------------------------------
MODES = {"fixed": {}, "fixed_pw": dict(primal_update=True), "adaptive": dict(adaptive=True),
         "adaptive_pw": dict(adaptive=True, primal_update=True)}


@pytest.mark.parametrize("W", [8, 16, 32])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mode", list(MODES))
def test_equal_columns_give_the_bits_of_the_shared_matrix(mode, dtype, W):
    B = 9
    f = family(B, seed=70, noise=0.0, dtype=dtype)
    K = csr(f)
    d = lambda v: v.to(dev())
    sigma = norm2(f, f.val)
    args = (K, f.m_ineq, d(f.C), d(f.Q), d(f.L), d(f.U), dev())
    kw = dict(sigma=sigma, group_width=W, max_kkt=3000, **MODES[mode])
    ra, rb = {}, {}
    a = pdlp_algorithm_batch(*args, report=ra, **kw)
    b = pdlp_algorithm_batch(*args, report=rb, K_values=K.val.view(-1, 1).repeat(1, B), **kw)
    assert_same_solve(a, ra, b, rb, what=f"{mode} W={W}")
    assert int(a[3].max()) >= 80                                  # more than one restart period was compared


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_equal_columns_give_the_bits_of_the_shared_matrix_ruiz(dtype):
    """the un-scaling epilogues (KKT pass and report) with the factors once shared, once as B equal columns"""
    B = 5
    f = family(B, seed=71, noise=0.0, dtype=dtype)
    K = csr(f)
    Ks, scaling = equilibrate_matrix(K, device=dev())
    dp = (scaling.d_col, scaling.d_row)
    Dc, Dr = dp[0].view(-1, 1), dp[1].view(-1, 1)
    sc = (f.C.to(dev()) * Dc, f.Q.to(dev()) * Dr, f.L.to(dev()) / Dc, f.U.to(dev()) / Dc)
    kw = dict(sigma=norm2(f, Ks.val.cpu()), precondition=True, adaptive=True, primal_update=True, max_kkt=3000)
    ra, rb = {}, {}
    a = pdlp_algorithm_batch(Ks, f.m_ineq, *sc, dev(), data_precond=dp, report=ra, **kw)
    b = pdlp_algorithm_batch(Ks, f.m_ineq, *sc, dev(), data_precond=(Dc.repeat(1, B), Dr.repeat(1, B)), report=rb,
                             K_values=Ks.val.view(-1, 1).repeat(1, B), KT_values=Ks.t_val.view(-1, 1).repeat(1, B), **kw)
    assert_same_solve(a, ra, b, rb, what="ruiz")


@pytest.mark.parametrize("mode", ["fixed", "adaptive_pw"])
@pytest.mark.parametrize("W", [8, 16, 32])
def test_an_lp_over_its_own_matrix_does_not_depend_on_its_batch(mode, W):
    """test_an_lp_does_not_depend_on_its_batch with a matrix per LP: LP b of the batch against a shared-matrix batch of that one
    LP over matrix b at the same W (its step size from the same sigma), and against the same LP at another position"""
    B = 8
    f = family(B, seed=72)
    assert not torch.equal(f.vals[:, 0], f.vals[:, 1])
    d = lambda v: v.to(dev())
    sig = np.array([norm2(f, f.vals[:, b]) for b in range(B)])
    kw = dict(group_width=W, max_kkt=2500, **MODES[mode])
    ra = {}
    a = pdlp_algorithm_batch(csr(f), f.m_ineq, d(f.C), d(f.Q), d(f.L), d(f.U), dev(), sigma=sig, report=ra, K_values=d(f.vals), **kw)
    for b in range(B):
        one = lambda v: d(v[:, b:b + 1])
        rb = {}
        alone = pdlp_algorithm_batch(csr(f, f.vals[:, b]), f.m_ineq, one(f.C), one(f.Q), one(f.L), one(f.U), dev(), sigma=float(sig[b]),
                                     report=rb, **kw)
        assert_same_solve(a, ra, alone, rb, cols_a=[b], cols_b=[0], what=f"{mode} LP {b}")
    perm = [5, 2, 7, 0, 3, 6, 1, 4, 2, 2]                          # another order, LP 2 three times: B = 10
    p = lambda v: d(v[:, perm])
    rc = {}
    c = pdlp_algorithm_batch(csr(f), f.m_ineq, p(f.C), p(f.Q), p(f.L), p(f.U), dev(), sigma=sig[perm], report=rc, K_values=p(f.vals), **kw)
    assert_same_solve(a, ra, c, rc, cols_a=perm, cols_b=list(range(len(perm))), what=f"{mode} permuted")


@pytest.mark.parametrize("mode", ["fixed", "adaptive_pw"])
def test_an_lp_over_its_own_matrix_float64(mode):
    """the same in float64 against shared-matrix batches of the SAME width: the driver takes ||q_b||, ||c_b|| from one torch
    reduction over the [len, B] array, whose float64 bits depend on B (float32 rounds that away) -- so here the shared-matrix batch
    over matrix b holds all B vector columns and column b is compared; every kernel launch is the one of the test above.
    (A float64 batch of ONE LP cannot be run at all: with B = 1, ``np.float64`` of the driver's one-element arrays gives scalars and
    ``BatchEngine.set_scalars`` / the rules raise IndexError -- README, "Batched solves", known limits.)"""
    B = 8
    f = family(B, seed=72, dtype=torch.float64)
    d = lambda v: v.to(dev())
    sig = np.array([norm2(f, f.vals[:, b]) for b in range(B)])
    kw = dict(group_width=8, max_kkt=2500, sigma=sig, **MODES[mode])
    ra = {}
    a = pdlp_algorithm_batch(csr(f), f.m_ineq, d(f.C), d(f.Q), d(f.L), d(f.U), dev(), report=ra, K_values=d(f.vals), **kw)
    for b in range(B):
        rb = {}
        over_b = pdlp_algorithm_batch(csr(f, f.vals[:, b]), f.m_ineq, d(f.C), d(f.Q), d(f.L), d(f.U), dev(), report=rb, **kw)
        assert_same_solve(a, ra, over_b, rb, cols_a=[b], cols_b=[b], what=f"{mode} LP {b}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. call by call against float64, LP by LP over that LP's matrix
# ---------------------------------------------------------------------------------------------------------------------------------
def noisy_values(va, B, rng, T):
    """[nnz, B] values of the working precision: column 0 the matrix itself, the others perturbed entry by entry, one entry in ten
    a stored zero in the odd columns"""
    V = np.stack([va.astype(np.float64)] + [va * (1 + 0.3 * rng.uniform(-1, 1, va.size)) for _ in range(1, B)], 1)
    V[::10, 1::2] = 0.0
    return V.astype(T)


class MBatch(bk.Batch):
    """tests.test_gpu_batch_kernels.Batch with a matrix (and Ruiz factors) per LP: ``Ps[b]`` is the LP of column b over its own
    matrix; the value and factor populations join the integer-view check of the frozen and padding columns"""

    def __init__(self, P, V, B, W=None, frozen=(), rng=None, D=None, eta_spread=(0.3, 3.0)):
        self.P, self.B, T = P, B, P.T
        self.Ps = [bk.LP(P.m, P.n, P.m_ineq, P.rp, P.ci, V[:, b], *P.vec, T=T) for b in range(B)]
        self.dt = TORCH[T]
        d = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev())
        dcol, drow = (None, None) if D is None else (d(D[0].astype(T)), d(D[1].astype(T)))
        self.be = be = BatchEngine(P.csr(), P.m_ineq, *(d(v) for v in P.vec), B, d_col=dcol, d_row=drow, W=W, K_values=d(V))
        self.Bp = be.Bp
        self.live = np.array([b for b in range(B) if b not in set(frozen)])
        self.dead = np.setdiff1d(np.arange(self.Bp), self.live)
        rng = np.random.default_rng(0) if rng is None else rng
        st = bk.random_state(P, self.Bp, self.live, rng, eta_spread)
        self.write(**st)
        pad = torch.from_numpy(np.arange(B, self.Bp)).to(dev())
        for v in [v for v in be.vec if v.dim() == 2] + self.matrices():          # padding columns of the per-LP data
            v[:, pad] = torch.from_numpy(bk.poison((v.shape[0], len(pad)), T)).to(dev())
        torch.cuda.synchronize()

    def matrices(self):
        be = self.be
        return [be.K_valB, be.KT_valB] + ([be.d_colB, be.d_rowB] if be.d_col is not None else [])

    def tensors(self):
        d = super().tensors()
        d.update({f"mat{i}": v for i, v in enumerate(self.matrices())})
        return d

    def pull(self):
        self.be.synchronize()
        torch.cuda.synchronize()
        idx = torch.from_numpy(self.live).to(dev())
        st = {k: v[..., idx].double().cpu().numpy() for k, v in bk.Batch.tensors(self).items() if not k.startswith("vec")}
        st["out"] = self.be.out[:, idx].cpu().numpy()
        for k in bk.XPOP + bk.YPOP + bk.SCAL:
            assert np.isfinite(st[k]).all(), f"a live column of {k} is not finite"
        return st

    def column(self, st, i):
        """(a stand-in for the batch that holds LP live[i] alone over its own matrix, the state of that column)"""
        b = int(self.live[i])
        one = types.SimpleNamespace(P=self.Ps[b], live=np.array([b]))
        return one, {k: (v[:, i:i + 1] if k == "out" else v[..., i:i + 1]) for k, v in st.items()}


def each_column(bt, check, *states_then_args, nstates=1):
    """run a checker of tests.test_gpu_batch_kernels LP by LP, each over its own matrix"""
    states, args = states_then_args[:nstates], states_then_args[nstates:]
    out = []
    for i in range(len(bt.live)):
        cols = [bt.column(s, i) for s in states]
        out.append(check(cols[0][0], *(c[1] for c in cols), *args))
    return out


def check_kkt_columns(bt, st, which, slot, u, D=None):
    for i, b in enumerate(bt.live):
        one, s = bt.column(st, i)
        bk.check_kkt(one, s, which, slot, u, None if D is None else (D[0][:, b], D[1][:, b]))


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_every_entry_point_call_by_call(T):
    """one fixed iteration, one adaptive iteration, the average, a KKT pass at each of CUR / AVG / PREV and the restart, every call
    from the state the last one left, frozen (3) and padding columns poisoned"""
    rng = np.random.default_rng(200)
    B = 9
    P, _ = bk.golden_lp(T, B, rng)
    V = noisy_values(P.va, B, rng, T)
    bt = MBatch(P, V, B, frozen=(3,), rng=rng, eta_spread=(0.2, 0.8))
    be, u = bt.be, bk.units(T)
    before, after = bt.call("iterate fixed", be.iterate, 1, False, 0)
    each_column(bt, bk.check_iterate, before, after, 1, False, 0, u, nstates=2)
    before, after = bt.call("iterate adaptive", be.iterate, 1, True, 3)
    each_column(bt, bk.check_iterate, before, after, 1, True, 3, u, nstates=2)
    before, after = bt.call("average adaptive", be.average, True)
    each_column(bt, bk.check_average, before, after, True, u, nstates=2)
    for which, slot in ((N.CUR, 0), (N.AVG, 1), (N.PREV, 2)):
        _, after = bt.call("kkt", be.kkt, which, slot)
        check_kkt_columns(bt, after, which, slot, u)
    actions = np.zeros(bt.Bp, np.int32)
    actions[bt.live] = np.arange(len(bt.live)) % 3
    bt.write(action=actions)
    before, after = bt.call("restart", be.restart, 1)
    each_column(bt, bk.check_restart, before, after, actions, 1, u, nstates=2)


def ruiz_batch(T, B, rng):
    """the golden ruiz.npz matrix and B - 1 perturbations of it, each equilibrated by the library: the scaled values, the factors
    (float64 copies of the working-precision numbers) and per-LP scaled vectors"""
    z = np.load(os.path.join(bk.GOLDEN, "ruiz.npz"))
    Kc = sp.csr_matrix(z["mixed_400x300/plain/it20/K"].astype(np.float64))
    Kc.sort_indices()
    m, n = Kc.shape
    t = lambda a, dt=TORCH[T]: torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dt)
    Kp = tp.CsrPair(m, n, t(Kc.indptr, torch.int64), t(Kc.indices, torch.int32), t(Kc.data)).to(dev())
    V0 = np.stack([Kc.data] + [Kc.data * (1 + 0.4 * rng.uniform(-1, 1, Kc.nnz)) for _ in range(1, B)], 1).astype(T)
    sv, stv, dc, dr, _ = ruiz_precondition_batch(Kp, t(V0).to(dev()))
    torch.cuda.synchronize()
    L, U = bk.bounds_mix(n, rng, np.float64, B)
    P = bk.LP(m, n, int(0.6 * m), Kc.indptr, Kc.indices, sv[:, 0].cpu().numpy(), rng.standard_normal((n, B)), rng.standard_normal((m, B)), L, U, T=T)
    return P, Kp, V0, sv, stv, dc, dr


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("which,slot", [(N.CUR, 0), (N.AVG, 2), (N.PREV, 1)], ids=["cur", "avg", "prev"])
@pytest.mark.parametrize("unscaled", [False, True], ids=["scaled", "unscaled"])
def test_kkt_with_ruiz_factors_per_lp(T, which, slot, unscaled):
    """test_kkt of tests/test_gpu_batch_kernels.py with a Ruiz-scaled matrix and factors per LP"""
    B = 11
    rng = np.random.default_rng(5)
    P, _, _, sv, _, dc, dr = ruiz_batch(T, B, rng)
    D = (dc.double().cpu().numpy(), dr.double().cpu().numpy())
    assert not np.allclose(D[0][:, 1], D[0][:, 2]) and not np.allclose(D[1], 1)
    bt = MBatch(P, sv.cpu().numpy(), B, frozen=(4,), rng=np.random.default_rng(slot), D=D)
    _, after = bt.call("kkt", bt.be.kkt, which, slot, unscaled)
    check_kkt_columns(bt, after, which, slot, bk.units(T), D if unscaled else None)
    other = [s for s in range(3) if s != slot]
    assert not after["out"][other].any(), "a KKT pass wrote another slot"


@pytest.mark.parametrize("unscaled", [0, 1])
@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_report_per_lp_against_float64_and_touches_nothing_else(T, unscaled):
    """test_batch_report_against_float64_and_touches_nothing_else (tests/test_gpu_report.py) with a matrix and factors per LP: its
    reference and bounds per column, its integer-view check of rc, act, out and every population"""
    rng = np.random.default_rng(23)
    B, Bp = 5, 8
    P0 = rp_.make_lp(T, rng, m=230, n=170, m_ineq=90)
    nnz = P0.va.size
    V = np.stack([P0.va] + [P0.va * (1 + 0.3 * rng.uniform(-1, 1, nnz)) for _ in range(1, B)], 1).astype(T)
    per = lambda v, ln, s=0.3: np.stack([v * (1 + s * rng.standard_normal(ln)) for _ in range(B)], 1).astype(T)
    Cb, Qb = per(P0.c, P0.n), per(P0.q, P0.m)
    Dc, Dr = np.abs(per(P0.dcol, P0.n, 0.1)), np.abs(per(P0.drow, P0.m, 0.1))
    Ps = [rp_.LP(P0.m, P0.n, P0.m_ineq, P0.rp, P0.ci, V[:, b], Cb[:, b], Qb[:, b], P0.l, P0.u, T, dcol=Dc[:, b], drow=Dr[:, b]) for b in range(B)]
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    be = BatchEngine(P0.csr(), P0.m_ineq, tt(Cb), tt(Qb), P0.vec("l"), P0.vec("u"), B, d_col=tt(Dc), d_row=tt(Dr), W=8, K_values=tt(V))
    assert be.Bp == Bp
    pops = {}
    for names, ln in ((bk.XPOP, P0.n), (bk.YPOP, P0.m)):
        for nm in names:
            v = rp_.poison((ln, Bp), T)
            v[:, :B] = torch.from_numpy(rng.uniform(-1, 1, (ln, B)).astype(T))
            getattr(be, nm).copy_(v)
            pops[nm] = getattr(be, nm).clone()
    for nm in bk.SCAL:
        getattr(be, nm).copy_(rp_.poison((Bp,), T))
        pops[nm] = getattr(be, nm).clone()
    for nm in ("K_valB", "KT_valB", "d_colB", "d_rowB"):
        v = getattr(be, nm)
        v[:, B:] = rp_.poison((v.shape[0], Bp - B), T).to(dev())
        pops[nm] = v.clone()
    live = np.zeros(Bp, np.int32)
    live[[0, 2]] = 1                              # LPs 1, 3, 4 are frozen and reported all the same; 5..7 are padding
    be.live.copy_(torch.from_numpy(live))
    be.out.copy_(rp_.poison((3, Bp, 6), np.float64))
    out0 = be.out.clone()
    torch.cuda.synchronize()
    u = np.finfo(T).eps
    iv = IVIEW[TORCH[T]]
    for slot, which in enumerate((N.CUR, N.AVG, N.PREV)):
        rc, act = rp_.poison((P0.n, Bp), T).to(dev()), rp_.poison((P0.m, Bp), T).to(dev())
        torch.cuda.synchronize()
        N.check(be.lib.pdlp_batch_report(be.eng.h, N.C.byref(be.desc), which, unscaled, slot, rc.data_ptr(), act.data_ptr()), "pdlp_batch_report")
        be.synchronize()
        out = be.out.cpu().numpy()
        X = rp_.h64(pops[("x", "x_avg", "x_prev")[which]]).reshape(P0.n, Bp)
        Y = rp_.h64(pops[("y", "y_avg", "y_prev")[which]]).reshape(P0.m, Bp)
        for b in range(B):
            lam, a, s, e_lam, e_act, bd = rp_.ref_report(Ps[b], X[:, b], Y[:, b], unscaled, u)
            rp_.assert_within(rp_.h64(rc[:, b]), lam, e_lam, f"reduced costs LP {b} which={which}")
            rp_.assert_within(rp_.h64(act[:, b]), a, e_act, f"row activity LP {b} which={which}")
            rp_.assert_within(out[slot, b], s, bd, f"sums LP {b} which={which}")
        assert torch.equal(rc[:, B:].contiguous().view(iv), rp_.poison((P0.n, Bp - B), T).to(dev()).view(iv))
        assert torch.equal(act[:, B:].contiguous().view(iv), rp_.poison((P0.m, Bp - B), T).to(dev()).view(iv))
        assert torch.equal(be.out[slot, B:].contiguous().view(torch.int64), out0[slot, B:].contiguous().view(torch.int64))
        assert torch.equal(be.out[slot + 1:].contiguous().view(torch.int64), out0[slot + 1:].contiguous().view(torch.int64))
        for nm, before in pops.items():            # every population and scalar, every column: the same bytes
            assert torch.equal(getattr(be, nm).view(iv), before.view(iv)), nm


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the plain product, the attach rules, the power iteration
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,W", [(np.float32, 8), (np.float32, 32), (np.float64, 16)], ids=["f32-W8", "f32-W32", "f64-W16"])
@pytest.mark.parametrize("per_lp", [False, True], ids=["shared", "per_lp"])
def test_population_product_against_float64(T, W, per_lp):
    rng = np.random.default_rng(W + per_lp)
    B = 10
    P = bk.shape_lp("long_row", T, B, "CQLU", rng)
    V = noisy_values(P.va, B, rng, T) if per_lp else np.repeat(P.va.astype(T)[:, None], B, 1)
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev())
    be = BatchEngine(P.csr(), P.m_ineq, *(d(v) for v in P.vec), B, W=W, K_values=d(V) if per_lp else None)
    u = bk.units(T)
    for transpose, rows_in, rows_out in ((False, P.n, P.m), (True, P.m, P.n)):
        Vin = bk.poison((rows_in, be.Bp), T)
        Vin[:, :B] = rng.uniform(-1, 1, (rows_in, B))
        out = be.product(d(Vin), transpose)
        be.synchronize()
        got = out.double().cpu().numpy()
        assert not got[:, B:].any(), "a padding column of the product was written"
        for b in range(B):
            Pb = bk.LP(P.m, P.n, P.m_ineq, P.rp, P.ci, V[:, b], *P.vec, T=T)
            M, Ma, L = (Pb.KT, Pb.KTa, Pb.Lc) if transpose else (Pb.K, Pb.Ka, Pb.Lr)
            x = Vin[:, b].astype(np.float64)
            bk.close(f"product transpose={transpose} LP {b}", got[:, b], M @ x, bk.gam(L, u) * (Ma @ np.abs(x)))
    one = torch.zeros(P.n, be.Bp, dtype=TORCH[T], device=dev())
    assert be.lib.pdlp_batch_product(be.eng.h, N.C.byref(be.desc), 0, one.data_ptr(), None) == -1
    assert be.lib.pdlp_batch_product(be.eng.h, N.C.byref(be.desc), 0, one.data_ptr(), one.data_ptr()) == -1


def test_attached_matrices_must_match_the_batch_width():
    rng = np.random.default_rng(3)
    P = bk.shape_lp("odd_rows", np.float32, 4, "CQLU", rng)
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev())
    be = BatchEngine(P.csr(), P.m_ineq, *(d(v) for v in P.vec), 4, W=8)
    lib, h = be.lib, be.eng.h
    wide = torch.ones(P.va.size, 16, device=dev())
    assert lib.pdlp_batch_attach_matrices(h, 16, wide.data_ptr(), None, None, None) == -1          # K without K'
    assert lib.pdlp_batch_attach_matrices(h, 16, wide.data_ptr(), wide.data_ptr(), wide.data_ptr(), None) == -1   # one factor
    assert lib.pdlp_batch_attach_matrices(h, 12, wide.data_ptr(), wide.data_ptr(), None, None) == -1
    assert lib.pdlp_batch_attach_matrices(h, 16, wide.data_ptr(), wide.data_ptr(), None, None) == 0
    assert lib.pdlp_batch_iterate(h, N.C.byref(be.desc), 1, 0, 0) == -1                             # Bp = 8 against 16 attached
    assert lib.pdlp_batch_kkt(h, N.C.byref(be.desc), 0, 0, 0) == -1
    assert lib.pdlp_batch_attach_matrices(h, 0, None, None, None, None) == 0                        # detached: the shared matrix again
    be.start(np.full(4, 0.01, np.float32), np.ones(4, np.float32))
    be.iterate(1, False, 0)
    be.synchronize()


def power_iteration_float64(K, b0, u, Lr, Lc, iters=100):
    """the reference's recurrence in float64 -> (sigma, a bound of what arithmetic with unit u does to it).

    Direction.  An iteration b -> A b / ||A b|| (A = K'K) commits a relative error e_k: the two products' running-error bounds
    (the product tolerance of tests/test_gpu_batch_kernels.py, carried through |K'|) over ||A b||, plus the norm and the division,
    (n + 4) u.  It carries the error E it received through the differential of the normalised map, (I - b b') A / ||A b||, whose
    norm is at most g_k = max(1, lam1 ||b|| / ||A b||): E <- g_k E + e_k.  g_k is 1 once the Rayleigh quotient has settled (the
    product of all g_k is 15 to 61 on the test's family).  lam1 = ||K||_2^2 is taken as the reference's own final estimate plus
    1e-5 relative: after 100 steps it is within 3e-7 relative of the dense 2-norm on every matrix of that family.
    Value.  sigma^2 = b'A b for unit b, and for the unit vector along b + d:  (b + d)'A (b + d) - rho ||b + d||^2 =
    2 d'(A b - rho b) + d'(A - rho) d  with rho = b'A b,  so  |sigma~^2 - sigma^2| <= (2 E R + lam1 E^2) / (1 - E)^2  with the
    eigen-residual R = ||A b - rho b||: the estimate is stationary at a converged direction, and the direction's error enters
    almost only in second order.  The last product and norm add their own running-error bound."""
    Ka, KT, KTa = abs(K), K.T.tocsr(), abs(K).T.tocsr()

    def run(lam1):
        b, E = b0.astype(np.float64), 0.0
        for _ in range(iters):
            t = K @ b
            e_t = bk.gam(Lr, u) * (Ka @ np.abs(b))
            v = KT @ t
            e_v = KTa @ e_t + bk.gam(Lc, u) * (KTa @ np.abs(t))
            nv, nb = np.linalg.norm(v), np.linalg.norm(b)
            E = max(1.0, lam1 * nb / nv) * E + np.linalg.norm(e_v) / nv + (len(v) + 4) * u
            b = v / nv
        return b, E

    b, _ = run(0.0)
    t = K @ b
    sigma = np.linalg.norm(t)
    lam1 = sigma * sigma * (1 + 1e-5)
    _, E = run(lam1)
    Ab = KT @ t
    R = np.linalg.norm(Ab - (b @ Ab) * b)
    assert E < 0.1
    value = (2 * E * R + lam1 * E * E) / ((1 - E) ** 2 * sigma)
    last = np.linalg.norm(bk.gam(Lr, u) * (Ka @ np.abs(b))) * (1 + E) + (len(t) + 4) * u * sigma
    return sigma, value + last


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_sigma_per_lp_against_a_float64_power_iteration(T):
    B = 6
    f = family(B, seed=73, noise=0.3, dtype=TORCH[T])
    d = lambda v: v.to(dev())
    be = BatchEngine(csr(f), f.m_ineq, d(f.C), d(f.Q), d(f.L), d(f.U), B, K_values=d(f.vals))
    g = torch.Generator().manual_seed(5)
    b0 = torch.randn(f.n, generator=g, dtype=torch.float32)
    got = estimate_sigma_batch(be, b0, 100)
    short = estimate_sigma_batch(be, b0, 10)                      # a wrong step count, which the bound must tell apart
    assert got.shape == (B,) and len(set(got.tolist())) == B
    Lr = np.diff(f.rowptr.numpy()).astype(np.float64)
    Lc = np.bincount(f.colidx.numpy(), minlength=f.n).astype(np.float64)
    told_apart = 0
    for b in range(B):
        K = sp.csr_matrix((f.vals[:, b].double().numpy(), f.colidx.numpy().copy(), f.rowptr.numpy().copy()), shape=(f.m, f.n))
        want, bound = power_iteration_float64(K, b0.numpy(), bk.units(T), Lr, Lc)
        print(f"LP {b}: sigma {got[b]!r} want {want!r} |diff| {abs(got[b] - want):.3e} bound {bound:.3e}")
        assert bk.C_BOUND * bound <= (1e-3 if T == np.float32 else 1e-12) * want         # the bound is one that binds
        bk.close(f"sigma of LP {b}", got[b], want, bound)
        told_apart += abs(short[b] - want) > bk.C_BOUND * bound
        other = (b + 1) % B                                       # nor does another LP's matrix pass for this one
        assert abs(got[other] - want) > bk.C_BOUND * bound, (b, other)
    assert told_apart >= B - 1, told_apart                        # (LP 0 has all but converged after 10 steps)
    # the start step of every LP is 0.9 / its own sigma (pdhg.py:22)
    drv = tp.BatchDriver(be, np.ones(B), np.ones(B))
    drv.start(got)
    be.synchronize()
    t = np.float32 if T == np.float32 else np.float64
    assert np.array_equal(be.eta[:B].cpu().numpy(), t(0.9) / got.astype(t))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. Ruiz per LP
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ruiz_per_lp_equals_ruiz_of_each_matrix_and_solves_like_solve_lp():
    B = 8
    f = family(B, seed=40)
    K = csr(f)
    sv, stv, dc, dr, secs = ruiz_precondition_batch(K, f.vals.to(dev()))
    for b in range(B):
        Ks, scaling = equilibrate_matrix(csr(f, f.vals[:, b]), device=dev())
        assert torch.equal(sv[:, b], Ks.val) and torch.equal(stv[:, b], Ks.t_val), b
        assert torch.equal(dc[:, b], scaling.d_col) and torch.equal(dr[:, b], scaling.d_row), b
    assert not torch.equal(dc[:, 0], dc[:, 1])
    prob = (f.C[:, 0], K, f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0])
    times = {}
    res = tp.solve_lp_batch(prob, f.C, f.Q, f.L, f.U, device=dev(), precondition=True, seed=0, K_values=f.vals, setup_times=times)
    assert times["ruiz_seconds"] > 0 and times["power_iteration_seconds"] > 0
    for b in range(B):                        # as test_ruiz_matches_solve_lp compares
        one = tp.solve_lp((f.C[:, b].to(dev()), csr(f, f.vals[:, b]), f.Q[:, b].to(dev()), f.m_ineq, f.L[:, b].to(dev()), f.U[:, b].to(dev())),
                          device=dev(), precondition=True, seed=0)
        assert res.status[b] == one.status
        assert abs(res.objective[b] - one.objective) <= 2e-3 * (1 + abs(one.objective)), b
        x, y = res.x[:, b].double().cpu().numpy(), res.y[:, b].double().cpu().numpy()
        xo = one.x.view(-1).double().cpu().numpy()
        assert np.linalg.norm(x - xo) <= 2e-2 * (1 + np.linalg.norm(xo)), b
        assert (y[:f.m_ineq] >= 0).all(), b
    # x and y come back un-scaled per LP: the scaled batch multiplied out on the host
    Xs, Ys, *_ = pdlp_algorithm_batch(K, f.m_ineq, f.C.to(dev()) * dc, f.Q.to(dev()) * dr, f.L.to(dev()) / dc, f.U.to(dev()) / dc, dev(),
                                      precondition=True, data_precond=(dc, dr), seed=0, K_values=sv, KT_values=stv)
    assert torch.equal(res.x, dc * Xs) and torch.equal(res.y, dr * Ys)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. end to end
# ---------------------------------------------------------------------------------------------------------------------------------
E2E = dict(B=33, seed=65, noise=0.2, max_kkt=100_000)


def test_matrix_noise_family_end_to_end():
    """float32, B = 33 (W = 32, two groups, 31 padding columns), every LP over its own matrix, to 1e-4.  Off the GPU, the float32
    CPU oracle's pdlp_algorithm (b0 of seed 0) reaches "Solved" on all 33 LPs of this family within max_kkt = 100000 (at most 17701
    passes on any LP), and its own objectives lie within 0.21 of this test's tolerance of the built-in optima: demanding "Solved"
    and the optimum of every LP hides no limit of the method.  That is a property of this seed.  The reference's signed-gap test
    at tol 1e-4 bounds the objective's error by tol (1 + |p| + |d|), which on an LP whose optimum is near 0 exceeds
    2e-3 (1 + |opt|); families of other seeds hold such an LP and the oracle itself then misses this tolerance on it (the reason
    test_widths_solve_every_lp scales by the size of the objective's terms).  Each objective against the built-in optimum
    c_b'X_opt[:, b], against solve_lp on that LP alone and, where scipy has it, against HiGHS on the first eight LPs, at the
    tolerance of test_width_32_float32_solves_like_solve_lp."""
    f = family(E2E["B"], seed=E2E["seed"], noise=E2E["noise"])
    B = f.B
    K = csr(f)
    prob = (f.C[:, 0], K, f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0])
    res = tp.solve_lp_batch(prob, f.C, f.Q, f.L, f.U, device=dev(), seed=0, K_values=f.vals, max_kkt=E2E["max_kkt"])
    assert res.status == ["Solved"] * B
    try:
        from scipy.optimize import linprog
    except ImportError:
        linprog = None
    judged = 0
    for b in range(B):
        opt = float((f.C[:, b].double() * f.X_opt[:, b].double()).sum())
        print(f"LP {b}: objective {res.objective[b]!r} optimum {opt!r}")
        assert abs(res.objective[b] - opt) <= 2e-3 * (1 + abs(opt)), b
        one = tp.solve_lp((f.C[:, b].to(dev()), csr(f, f.vals[:, b]), f.Q[:, b].to(dev()), f.m_ineq, f.L[:, b].to(dev()), f.U[:, b].to(dev())),
                          device=dev(), seed=0)
        assert one.status == "Solved"
        assert abs(res.objective[b] - one.objective) <= 2e-3 * (1 + abs(one.objective)), b
        Kd = dense(f, f.vals[:, b])
        x = res.x[:, b].double().cpu().numpy()
        q = f.Q[:, b].double().numpy()
        r = Kd @ x - q
        viol = np.concatenate([np.minimum(r[:f.m_ineq], 0), r[f.m_ineq:]])
        assert np.linalg.norm(viol) <= 1.5e-4 * (1 + np.linalg.norm(q)), b               # feasible for ITS matrix
        if linprog is not None and b < 8:
            c, l, u = (v[:, b].double().numpy() for v in (f.C, f.L, f.U))
            bounds = [(None if np.isinf(a) else a, None if np.isinf(z) else z) for a, z in zip(l, u)]
            h = linprog(c, A_ub=-Kd[:f.m_ineq], b_ub=-q[:f.m_ineq], A_eq=Kd[f.m_ineq:], b_eq=q[f.m_ineq:], bounds=bounds, method="highs")
            if h.status != 0:             # (as test_mps_family_against_highs: float32-rounded data can defeat its presolve)
                continue
            assert abs(res.objective[b] - h.fun) <= 2e-3 * (1 + abs(h.fun)), (b, res.objective[b], h.fun)
            judged += 1
    assert linprog is None or judged > 0, "HiGHS solved none of the LPs it was given"


def test_matrix_noise_family_against_highs():
    """a float64 family (its optima are exact, so HiGHS solves every LP) through the union-pattern helper"""
    opt = pytest.importorskip("scipy.optimize")
    f = family(8, seed=62, noise=0.25, n=120, m=90, dtype=torch.float64)
    K = tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val)
    pattern, vals = tp.stack_matrices([K.with_values(f.vals[:, b].contiguous()) for b in range(f.B)])
    res = tp.solve_lp_batch((f.C[:, 0], pattern, f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0]), f.C, f.Q, f.L, f.U, device=dev(), seed=0,
                            K_values=vals, dtype=torch.float64)
    for b in range(f.B):
        Kd = dense(f, f.vals[:, b])
        c, q, l, u = (v[:, b].double().numpy() for v in (f.C, f.Q, f.L, f.U))
        bounds = [(None if np.isinf(a) else a, None if np.isinf(z) else z) for a, z in zip(l, u)]
        h = opt.linprog(c, A_ub=-Kd[:f.m_ineq], b_ub=-q[:f.m_ineq], A_eq=Kd[f.m_ineq:], b_eq=q[f.m_ineq:], bounds=bounds, method="highs")
        assert h.status == 0
        assert res.status[b] == "Solved", b
        assert abs(res.objective[b] - h.fun) <= 2e-3 * (1 + abs(h.fun)), (b, res.objective[b], h.fun)
