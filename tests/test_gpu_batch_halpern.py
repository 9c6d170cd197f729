"""The reflected Halpern iteration per LP of a batch on the MI355X (pdlp_batch_halpern_iterate, BatchEngine.halpern_iterate,
pdlp_algorithm_batch / solve_lp_batch(halpern=True)).

Every stored value of an iteration is pinned bit for bit against code already in the tree: the candidate and xbar against one fixed
step of ``pdlp_batch_iterate`` from the same state, the combination against separate torch elementwise operations with the weights
of ``rules.halpern_weights`` (the library is built without contraction, so these are the kernel's roundings).  Whole solves are
compared with ``run_pdlp(halpern=True)`` on one ``PdlpEngine`` per LP, with known optima, and with the plain batch when streamed."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import torchpdlp_amd as tp
from tests import test_gpu_batch_kernels as bk
from tests import test_gpu_batch_stream as bs
from tests.test_gpu_batch_matrices import MBatch, noisy_values
from torchpdlp_amd import _native as N
from torchpdlp_amd.batch import pdlp_algorithm_batch
from torchpdlp_amd.rules import halpern_weights
from torchpdlp_amd.solver import run_pdlp

pytestmark = pytest.mark.gpu

T_SINCE = [0, 1, 39, 40, 10**6 + 1, 2**31 + 5]
UNTOUCHED = ("x_prev", "y_prev", "x_sum", "y_sum", "dy", "eta_sum", "wpend")
WRITTEN = ("x", "xbar", "x_avg", "y", "y_avg")
CASES = ["ineq0", "ineq_all", "odd_rows", "tiny_2x3", "mixed_400x300", "k_values"]


def dev():
    return torch.device("cuda", 0)


def make_batch(case, T, B, W, rng, frozen=()):
    """a batch with a random state in the live columns: the edge shapes with per-LP and shared vectors, bounds of every class
    (infinite on either side and on both), the golden 400 x 300 LP, and one batch with a matrix per LP"""
    if case == "tiny_2x3":                       # fewer rows than a wave covers at any W
        rp, ci, _ = bk.csr_of_rows(2, 3, [[0, 2], [1]], np.zeros(0))
        va = rng.uniform(0.2, 2.0, ci.size) * rng.choice([-1, 1], ci.size)
        L, U = bk.bounds_mix(3, rng, np.float64, B)
        P = bk.LP(2, 3, 1, rp, ci, va, rng.standard_normal((3, B)), rng.standard_normal((2, B)), L, U, T=T)
    elif case == "mixed_400x300":
        P, _ = bk.golden_lp(T, B, rng)
    elif case == "k_values":
        P = bk.shape_lp("odd_rows", T, B, "CQLU", rng)
        return MBatch(P, noisy_values(P.va, B, rng, T), B, W=W, frozen=frozen, rng=rng)
    else:
        P = bk.shape_lp(case, T, B, {"ineq0": "CQLU", "ineq_all": "cQlu", "odd_rows": "CqLU"}[case], rng)
    return bk.Batch(P, B, W=W, frozen=frozen, rng=rng)


def t_since_of(bt, shift=0):
    """[Bp] int64: the values of T_SINCE in turn over the columns, so that the columns of one group differ"""
    ts = np.zeros(bt.Bp, np.int64)
    ts[:bt.B] = [T_SINCE[(b + shift) % len(T_SINCE)] for b in range(bt.B)]
    return ts


def restore(bt, snap):
    bt.be.synchronize()
    for k, v in bt.tensors().items():
        v.copy_(snap[k])
    torch.cuda.synchronize()


def same_bits(a, b):
    return torch.equal(a.view(bk.IVIEW[a.dtype]), b.view(bk.IVIEW[b.dtype]))


def weights(bt, ts):
    """(a, bw) of every live column as [live] tensors of the working type, from rules.halpern_weights"""
    w = [halpern_weights(int(ts[b]), bt.P.T) for b in bt.live]
    return tuple(torch.from_numpy(np.array([v[i] for v in w], bt.P.T)).to(dev()) for i in (0, 1))


def chain_step(bt, ts):
    """one Halpern iteration built from trusted code, from the state the batch holds: one fixed step of pdlp_batch_iterate gives
    x', xbar and y'; the two combinations are separate torch multiplications and additions in the working type.  The batch is left
    as it was.  -> dict of the five stored populations, live columns only"""
    be = bt.be
    idx = torch.from_numpy(bt.live).to(dev())
    snap = snapshot(bt)
    be.iterate(1, False, 0)
    be.synchronize()
    cand = {"x_avg": be.x[:, idx].clone(), "xbar": be.xbar[:, idx].clone(), "y_avg": be.y[:, idx].clone()}
    restore(bt, snap)
    a, bw = weights(bt, ts)
    p1, p2 = a * cand["xbar"], bw * be.x_last[:, idx]
    cand["x"] = p1 + p2
    r = torch.full_like(a, 2) * cand["y_avg"]
    r = r - be.y[:, idx]
    p1, p2 = a * r, bw * be.y_last[:, idx]
    cand["y"] = p1 + p2
    torch.cuda.synchronize()
    return cand


def live_part(bt, names=WRITTEN):
    idx = torch.from_numpy(bt.live).to(dev())
    bt.be.synchronize()
    out = {nm: getattr(bt.be, nm)[:, idx].clone() for nm in names}
    torch.cuda.synchronize()
    return out


def assert_step(bt, got, want, what):
    for nm in WRITTEN:
        assert torch.equal(got[nm], want[nm]), f"{what}: {nm} differs in {int((got[nm] != want[nm]).sum())} entries"
        assert bool(torch.isfinite(got[nm]).all()), f"{what}: {nm} is not finite"


def assert_rest_unchanged(bt, snap, what):
    """everything the call must not touch, of EVERY column, and every byte of the frozen and padding columns"""
    bt.be.synchronize()
    for k, v in bt.tensors().items():
        if k not in WRITTEN:
            assert same_bits(snap[k], v), f"{what}: {k} was written"
    assert same_bits(snap["part"], bt.be.part), f"{what}: the partial sums were written"
    bt.dead_unchanged(snap, what)


def snapshot(bt):
    bt.be.synchronize()
    snap = bt.snapshot()
    snap["part"] = bt.be.part.clone()
    torch.cuda.synchronize()
    return snap


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. one iteration
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("W", [8, 16, 32])
@pytest.mark.parametrize("dB", [-3, 0, 1], ids=["W-3", "W", "W+1"])
@pytest.mark.parametrize("case", CASES)
def test_one_iteration_bit_for_bit(T, W, dB, case):
    B = W + dB
    rng = np.random.default_rng(1000 * CASES.index(case) + 10 * W + dB + (T == np.float64))
    bt = make_batch(case, T, B, W, rng)
    assert bt.be.W == W and bt.Bp == (W if dB <= 0 else 2 * W)
    ts = t_since_of(bt, shift=CASES.index(case))
    want = chain_step(bt, ts)
    snap = snapshot(bt)
    bt.be.halpern_iterate(1, ts)
    got = live_part(bt)
    assert_step(bt, got, want, f"{case} B={B} W={W}")
    assert_rest_unchanged(bt, snap, f"{case} B={B} W={W}")
    # the candidate is inside the bounds, the reflected iterate need not be
    for i, b in enumerate(bt.live[:3]):
        c, q, l, u = bt.P.col(b)
        xc, yc = got["x_avg"][:, i].double().cpu().numpy(), got["y_avg"][:, i].double().cpu().numpy()
        assert (xc >= l).all() and (xc <= u).all() and (yc[:bt.P.m_ineq] >= 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. three iterations in one call, in three calls, and as a chain
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case,B,W", [("mixed_400x300", 9, 8), ("odd_rows", 13, 16), ("k_values", 33, 32)])
def test_three_iterations_in_one_call(T, case, B, W):
    rng = np.random.default_rng(7 + B)
    bt = make_batch(case, T, B, W, rng)
    ts = t_since_of(bt, shift=2)
    start = snapshot(bt)
    bt.be.halpern_iterate(3, ts)
    one = snapshot(bt)
    restore(bt, start)
    for it in range(3):
        bt.be.halpern_iterate(1, ts + it)
    three = snapshot(bt)
    for k in one:
        assert same_bits(one[k], three[k]), k
    restore(bt, start)
    idx = torch.from_numpy(bt.live).to(dev())
    for it in range(3):
        want = chain_step(bt, ts + it)
        for nm in WRITTEN:
            getattr(bt.be, nm)[:, idx] = want[nm]
        torch.cuda.synchronize()
    got = live_part(bt)
    for nm in WRITTEN:
        assert torch.equal(got[nm], one[nm][:, idx]), nm
    assert_rest_unchanged(bt, one, "the chain")            # (and the chain left everything else as the call did)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. frozen and padding columns
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case,B,W", [("mixed_400x300", 10, 8), ("ineq_all", 12, 16), ("k_values", 11, 8)])
def test_frozen_and_padding_columns(T, case, B, W):
    """columns 1 and 6 are frozen, the padding columns follow B: all hold the poison pattern before the call and after it; the
    populations the iteration does not use keep every byte in every column"""
    rng = np.random.default_rng(17 + B)
    bt = make_batch(case, T, B, W, rng, frozen=(1, 6))
    assert len(bt.dead) == bt.Bp - B + 2
    ts = t_since_of(bt)
    want = chain_step(bt, ts)
    snap = snapshot(bt)
    before, after = bt.call("halpern_iterate", bt.be.halpern_iterate, 1, ts)
    assert_step(bt, live_part(bt), want, case)
    assert_rest_unchanged(bt, snap, case)
    for nm in UNTOUCHED + ("x_last", "y_last", "eta", "omega"):
        assert np.array_equal(before[nm], after[nm]), nm
    bt.be.halpern_iterate(4, ts + 1)
    assert_rest_unchanged(bt, snap, f"{case}, four more")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. arguments
# ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    rng = np.random.default_rng(4)
    bt = make_batch("odd_rows", np.float32, 9, 8, rng)
    be = bt.be
    ts = torch.zeros(bt.Bp, dtype=torch.int64, device=dev())
    call = lambda desc, iters, p: be.lib.pdlp_batch_halpern_iterate(be.eng.h, desc, iters, p)
    snap = snapshot(bt)
    assert call(C.byref(be.desc), 1, None) == -1
    assert call(C.byref(be.desc), -1, ts.data_ptr()) == -1
    assert call(None, 1, ts.data_ptr()) == -1
    assert be.lib.pdlp_batch_halpern_iterate(None, C.byref(be.desc), 1, ts.data_ptr()) == -1
    bad = N.PdlpBatch.from_buffer_copy(be.desc)
    bad.W = 12
    assert call(C.byref(bad), 1, ts.data_ptr()) == -1
    assert call(C.byref(be.desc), 0, ts.data_ptr()) == 0
    be.halpern_iterate(0, np.zeros(9, np.int64))
    be.synchronize()
    for k, v in bt.tensors().items():
        assert same_bits(snap[k], v), k
    with pytest.raises(N.PdlpError, match="invalid"):
        be.halpern_iterate(-2, np.zeros(9, np.int64))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. whole solves in float64 against run_pdlp(halpern=True) LP by LP
# ---------------------------------------------------------------------------------------------------------------------------------
def perturbed_family(name, B=5, seed=0):
    g = np.load(os.path.join(bk.GOLDEN, "solve_trace.npz"))
    a = lambda k: g[f"{name}/{k}"]
    rng = np.random.default_rng(seed)
    m, n = int(a("m")), int(a("n"))
    c0, q0 = a("c").astype(np.float64), a("q").astype(np.float64)
    Cm = np.stack([c0] + [c0 * (1 + 0.05 * rng.standard_normal(n)) for _ in range(1, B)], 1)
    # (right-hand sides that keep every LP feasible: the inequality rows K x >= q are loosened, the equality rows stay)
    ineq = np.arange(m) < int(a("m_ineq"))
    Qm = np.stack([q0] + [q0 - ineq * 0.05 * (1 + np.abs(q0)) * np.abs(rng.standard_normal(m)) for _ in range(1, B)], 1)
    h = lambda v, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(v)).to(dtype=dt)
    t = lambda v: h(v).to(dev())
    K = tp.CsrPair(m, n, h(a("rowptr"), torch.int64), h(a("colidx"), torch.int32), h(a("val"))).to(dev())
    sigma = float(g[f"{name}/fixed_nopw/sigma"])
    return K, int(a("m_ineq")), t(Cm), t(Qm), t(a("l")), t(a("u")), sigma


@functools.lru_cache(maxsize=None)
def single_solves(name, pw, max_kkt):
    K, m_ineq, Cm, Qm, l, u, sigma = perturbed_family(name)
    out = []
    for b in range(Cm.shape[1]):
        eng = tp.PdlpEngine.from_full(K, Cm[:, b].contiguous(), Qm[:, b].contiguous(), l, u, m_ineq)
        trace = dict(kkt=[], omega=[], restarts=[])
        x, obj, k, n, j, status, _ = run_pdlp(eng, max_kkt=max_kkt, tol=1e-4, verbose=False, primal_update=pw, sigma=sigma, trace=trace,
                                              halpern=True)
        out.append((x.clone(), obj, k, n, j, status, trace))
        del eng
    return out


@pytest.mark.parametrize("name", ["mixed_27x32", "mixed_400x300"])
@pytest.mark.parametrize("pw", [False, True], ids=["nopw", "pw"])
def test_whole_solves_float64_against_the_single_lp_driver(name, pw):
    """(k, n, j), status and the restart list per LP are equal; the kkt and omega traces agree to rtol = 1e-9, compare_solves'
    tolerance for the averaged method.  The solves run to the default tol = 1e-4, as the whole solves compare_solves judges do:
    the two drivers sum a row's products in different orders, which moves a residual of O(1)..O(10) data by some 1e-14 in
    float64, and only KKT errors of 1e-5 and more can then agree to a relative 1e-9."""
    max_kkt = 20_000
    ref = single_solves(name, pw, max_kkt)
    K, m_ineq, Cm, Qm, l, u, sigma = perturbed_family(name)
    B = Cm.shape[1]
    traces = [dict(kkt=[], omega=[], restarts=[]) for _ in range(B)]
    X, Y, obj, k, n, j, status, _ = pdlp_algorithm_batch(K, m_ineq, Cm, Qm, l, u, dev(), max_kkt=max_kkt, tol=1e-4, primal_update=pw,
                                                         sigma=sigma, traces=traces, halpern=True)
    assert status[0] == "Solved", status                   # (column 0 is the golden LP itself)
    for b, (xr, objr, kr, nr, jr, sr, tr) in enumerate(ref):
        print(f"{name} pw={pw} LP {b}: k={int(k[b])} n={int(n[b])} j={int(j[b])} {status[b]} (single: {kr} {nr} {jr} {sr})")
        assert (int(k[b]), int(n[b]), int(j[b]), status[b]) == (kr, nr, jr, sr), b
        assert [tuple(r) for r in traces[b]["restarts"]] == [tuple(r) for r in tr["restarts"]], b
        assert len(traces[b]["kkt"]) == len(tr["kkt"]), b
        np.testing.assert_allclose(traces[b]["kkt"], tr["kkt"], rtol=1e-9, err_msg=str(b))
        np.testing.assert_allclose(traces[b]["omega"], tr["omega"], rtol=1e-9, err_msg=str(b))
        checks = int(k[b]) // 40
        assert int(j[b]) == int(k[b]) + checks + 2 * int(n[b]), b


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. end to end in float32 against known optima
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "ruiz", "k_values"])
def test_family_end_to_end_float32(mode):
    """12 LPs with built-in optima (gen_lp_family), each judged against its own: "Solved", the report's relative residuals and gap
    within tol, the objective within 1e-3 (1 + |opt|).  The shape and tol come from that last bound.  A point that passes the
    exit test has a primal residual of at most tol (1 + ||q||), a dual residual of at most tol (1 + ||c||) and a gap of at most
    tol (1 + |p| + |d|), and these move c'x from the optimum by no more than about
    ||y_opt|| tol (1 + ||q||) + ||x_opt|| tol (1 + ||c||) + tol (1 + 2 |opt|).  The norms grow with the size of the LP: at
    300 x 240 this exceeds the bound unless tol < 1e-6, which float32 does not reach; at 40 x 30 (three workgroups per product at
    W = 16) tol = 1e-5 keeps it below the bound for every LP of the family, asserted below from the built-in optima alone."""
    B, tol = 12, 1e-5
    noise = 0.2 if mode == "k_values" else 0.0
    f = tp.gen_lp_family(40, 30, 4, B, seed=5, matrix_noise=noise)
    nrm = lambda v: np.linalg.norm(v.double().numpy(), axis=0)
    opt = np.asarray(f.opt_obj, np.float64)
    worst = tol * ((1 + nrm(f.Q)) * nrm(f.Y_opt) + (1 + nrm(f.C)) * nrm(f.X_opt) + 1 + 2 * np.abs(opt))
    assert (worst <= 1e-3 * (1 + np.abs(opt))).all(), "the family does not suit the objective's bound at this tol"
    K = tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val)
    prob = (f.C[:, 0], K, f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0])
    kw = dict(precondition=True) if mode == "ruiz" else dict(K_values=f.vals) if mode == "k_values" else {}
    res = tp.solve_lp_batch(prob, f.C, f.Q, f.L, f.U, device=dev(), tol=tol, halpern=True, primal_weight_update=True, seed=0, **kw)
    print(f"{mode}: k={res.iterations.tolist()} n={res.restarts.tolist()} j={res.kkt_passes.tolist()}")
    assert res.status == ["Solved"] * B, res.status
    for name in ("rel_primal_residual", "rel_dual_residual", "rel_gap"):
        assert (getattr(res, name) <= tol).all(), (name, getattr(res, name))
    print(f"{mode}: objective error / bound {(np.abs(res.objective - opt) / (1e-3 * (1 + np.abs(opt)))).round(3).tolist()}")
    assert (np.abs(res.objective - opt) <= 1e-3 * (1 + np.abs(opt))).all(), (res.objective, opt)
    checks = res.iterations // 40
    assert (res.kkt_passes == res.iterations + checks + 2 * res.restarts).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. streaming
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_streamed_family_has_the_bits_of_the_plain_batch(dtype):
    f = bs.family(20, seed=61, dtype=dtype)
    x0, y0 = bs.uneven_start(f)
    sig = bs.norm2(f)
    mode = dict(halpern=True, primal_update=True)
    plain, rp, _ = bs.solve(f, sigma=sig, x_init=x0, y_init=y0, **mode)
    streamed, rs, sched = bs.solve(f, slots=8, sigma=sig, x_init=x0, y_init=y0, **mode)
    assert plain[6] == ["Solved"] * 20 and len(set(plain[3].tolist())) > 2
    bs.assert_overlap(sched, streamed[3])
    bs.assert_same_solve(plain, rp, streamed, rs)


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the limits
# ---------------------------------------------------------------------------------------------------------------------------------
def test_time_limit_and_kkt_cap_between_checks():
    f = bs.family(16, seed=63)
    sig = bs.norm2(f)
    x0 = (0.5 * f.X_opt).float()
    for slots in (None, 8):                  # the clock has run out when the first columns have been admitted
        out, rep, _ = bs.solve(f, slots=slots, sigma=sig, x_init=x0, halpern=True, time_limit=0)
        assert out[6] == [bs.TIME_LIMIT] * 16 and (out[3] == 0).all() and (out[5] == 0).all(), slots
        assert torch.equal(out[0].cpu(), x0) and not bool(out[1].any()), slots
    # the cap falls between two checks (40 iterations and one check are 41 passes): the point kept is the candidate of the last
    # iteration, inside the bounds, never the reflected iterate
    out, rep, _ = bs.solve(f, sigma=sig, x_init=x0, halpern=True, max_kkt=50)
    X, Y = out[0].cpu(), out[1].cpu()
    k, n, j = out[3], out[4], out[5]
    assert out[6] == [bs.KKT_LIMIT] * 16 and (k % 40 != 0).all() and (j >= 50).all(), out[3:7]
    assert (j == k + k // 40 + 2 * n).all(), (k, n, j)
    assert bool((X >= f.L).all()) and bool((X <= f.U).all()) and bool((Y[:f.m_ineq] >= 0).all())
    assert not torch.equal(X, x0)
