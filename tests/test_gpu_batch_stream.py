"""A family streamed through a fixed set of columns on the MI355X (``solve_lp_batch(slots=...)``, pdlp_batch_iterate_from /
pdlp_batch_admit / pdlp_batch_retire): the streamed results are the plain batch's bit for bit, the three entry points write what
they say and nothing else, and the limits hold per LP (``max_kkt``) and per run (``time_limit``)."""
import ctypes as C

import numpy as np
import pytest
import torch

import torchpdlp_amd as tp
from torchpdlp_amd import _native as N
from torchpdlp_amd.batch import BatchEngine, pdlp_algorithm_batch

pytestmark = pytest.mark.gpu

TIME_LIMIT = "Unsolved (Time limit exceeded)"
KKT_LIMIT = "Unsolved (KKT passes limit exceeded)"


def dev():
    return torch.device("cuda", 0)


def family(B, seed=3, n=300, m=240, dtype=torch.float32, noise=0.0):
    return tp.gen_lp_family(n, m, 4, B, seed=seed, dtype=dtype, matrix_noise=noise)


def csr(f):
    return tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val).to(dev())


def norm2(f, vals=None):
    va = (f.val if vals is None else vals).double()
    return float(np.linalg.norm(torch.sparse_csr_tensor(f.rowptr, f.colidx.long(), va, (f.m, f.n)).to_dense().numpy(), 2))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(a, b):
    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and same_bits(a.cpu().numpy(), b.cpu().numpy())
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def uneven_start(f):
    """every third LP starts at its optimum (solved at its first check, k = 40), the others at 0: columns fall free at once"""
    x0, y0 = torch.zeros(f.n, f.B, dtype=f.C.dtype), torch.zeros(f.m, f.B, dtype=f.C.dtype)
    x0[:, ::3], y0[:, ::3] = f.X_opt[:, ::3].to(f.C.dtype), f.Y_opt[:, ::3].to(f.C.dtype)
    return x0, y0


def solve(f, slots=None, where=None, **kw):
    where = dev() if where is None else where
    d = lambda v: v.to(where)
    kw = {k: (d(v) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    rep, sched = {}, {}
    out = pdlp_algorithm_batch(csr(f), f.m_ineq, d(f.C), d(f.Q), d(f.L), d(f.U), dev(), report=rep, slots=slots, schedule=sched,
                               group_width=8, **kw)
    return out, rep, sched


def assert_same_solve(a, ra, b, rb):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for i, name in ((3, "k"), (4, "n"), (5, "j")):
        assert list(a[i]) == list(b[i]), name
    assert a[6] == b[6]
    assert same_bits(a[2], b[2]), "obj"
    for key in ("y", "reduced_costs", "row_activity"):
        assert torch.equal(ra[key], rb[key]), key
    for key in ("pr", "dr", "gap", "p", "d_adj", "kkt", "q_norm", "c_norm"):
        assert same_bits(ra[key], rb[key]), key


def assert_overlap(sched, k):
    """some LP entered at k_global > 0 while another column was still iterating -- else the run proves nothing about streaming"""
    adm = sched["admitted_at"]
    hit = [(i, j) for i in np.flatnonzero(adm > 0) for j in range(len(adm)) if j != i and 0 <= adm[j] < adm[i] < adm[j] + k[j]]
    assert hit, (adm, k)
    assert sorted(np.unique(sched["column"]).tolist()) == list(range(sched["slots"]))
    assert (sched["retired_at"] >= adm + k).all()


@pytest.mark.parametrize("mode", [dict(), dict(adaptive=True, primal_update=True)], ids=["fixed", "adaptive_pw"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_streamed_family_has_the_bits_of_the_plain_batch(mode, dtype):
    """N = 40 through 8 columns at W = 8 against the plain batch of all 40 at W = 8.  The adaptive rule is the case that fails when
    k_start is ignored: an LP admitted at k_global = 40 would use (k_global + 1)^-0.3 for its own first step."""
    f = family(40, seed=61, dtype=dtype)
    x0, y0 = uneven_start(f)
    sig = norm2(f)
    plain, rp, _ = solve(f, sigma=sig, x_init=x0, y_init=y0, **mode)
    streamed, rs, sched = solve(f, slots=8, sigma=sig, x_init=x0, y_init=y0, **mode)
    assert plain[6] == ["Solved"] * 40 and len(set(plain[3].tolist())) > 2          # uneven finishing, by construction
    assert (plain[3][::3] == 40).all()
    assert_overlap(sched, streamed[3])
    assert_same_solve(plain, rp, streamed, rs)


def started_engine(f, B=8, adaptive_warm=0, K_values=None):
    d = lambda v: v[:, :B].to(dev())
    be = BatchEngine(csr(f), f.m_ineq, d(f.C), d(f.Q), d(f.L), d(f.U), B, W=8, K_values=None if K_values is None else d(K_values))
    t = np.float32
    eta = (0.9 / norm2(f)) * np.linspace(0.7, 1.3, B).astype(t)
    be.start(eta.astype(t), np.linspace(0.5, 2.0, B).astype(t), d(f.X_opt).float() * 0.5, d(f.Y_opt).float() * 0.5)
    if adaptive_warm:
        be.iterate(adaptive_warm, True, 0)
    return be


def state(be):
    names = ("x", "x_prev", "xbar", "x_sum", "x_avg", "x_last", "y", "y_prev", "y_sum", "y_avg", "y_last", "dy", "eta", "omega",
             "eta_sum", "wpend", "live", "action")
    st = {k: getattr(be, k).cpu().numpy().copy() for k in names}
    for k, v in zip("cqlu", be.vec):
        st[k] = v.cpu().numpy().copy()
    if be.per_lp_matrices:
        st["K_valB"], st["KT_valB"] = be.K_valB.cpu().numpy().copy(), be.KT_valB.cpu().numpy().copy()
    be.synchronize()
    return st


def test_iterate_from_counts_each_column_from_its_admission():
    f = family(8, seed=62)
    iters = 40
    a = started_engine(f)
    a.iterate(iters, True, 0)
    fresh = state(a)                                     # every column counted from 0
    b = started_engine(f)
    b.iterate(iters, True, 80)
    late = state(b)                                      # every column counted from 80
    c = started_engine(f)
    c.enable_stream()
    ks = np.zeros(8, np.int64)
    ks[3] = 80
    c.set_scalars(k_start=ks)
    c.iterate(iters, True, 80)                           # pdlp_batch_iterate_from with k_start
    mixed = state(c)
    e = started_engine(f)
    N.check(e.lib.pdlp_batch_iterate_from(e.eng.h, C.byref(e.desc), iters, 1, 80, None))
    null = state(e)
    assert not same_bits(fresh["eta"][3], late["eta"][3])        # (the count matters to the rule at all)
    for key in fresh:
        cols = lambda v: v if v.ndim == 1 else v.T
        for col in range(8):
            want = fresh if col == 3 else late
            assert same_bits(cols(mixed[key])[col], cols(want[key])[col]), (key, col)
        assert same_bits(null[key], late[key]), key


@pytest.mark.parametrize("attached", [False, True], ids=["shared_K", "per_lp_values"])
def test_admit_writes_its_columns_and_nothing_else(attached):
    f = family(8, seed=63, noise=0.2 if attached else 0.0)
    be = started_engine(f, adaptive_warm=7, K_values=f.vals if attached else None)
    before = state(be)
    cols_0 = [5, 1]
    assert before["x_sum"][:, cols_0].any() and np.abs(before["wpend"]).min() > 0 and np.abs(before["eta_sum"]).min() > 0
    g = torch.Generator().manual_seed(9)
    Nf = 5
    r = lambda rows: torch.randn(rows, Nf, generator=g).to(dev())
    feed = dict(c=r(f.n), q=r(f.m), l=r(f.n) - 3, u=r(f.n) + 3, x0=r(f.n), y0=r(f.m))
    if attached:
        feed.update(K_val=r(be.K_valB.shape[0]), KT_val=r(be.K_valB.shape[0]))
    eta, omega = np.linspace(0.01, 0.05, Nf).astype(np.float32), np.linspace(3.0, 7.0, Nf).astype(np.float32)
    cols, ids = [5, 1], [3, 0]
    be.admit(cols, ids, eta, omega, **feed)
    after = state(be)
    T = lambda v: v if v.ndim == 1 else v.T                      # (column-major view: index = column)
    for key in before:
        for col in range(8):
            if col not in cols or key in ("x_prev", "xbar", "x_avg", "y_prev", "y_avg", "dy", "live", "action"):
                assert same_bits(T(after[key])[col], T(before[key])[col]), (key, col)
    h = {k: v.cpu().numpy() for k, v in feed.items()}
    for col, i in zip(cols, ids):
        for key in "cqlu":
            assert same_bits(after[key][:, col], h[key][:, i]), (key, col)
        for key, src in (("x", "x0"), ("x_last", "x0"), ("y", "y0"), ("y_last", "y0")):
            assert same_bits(after[key][:, col], h[src][:, i]), (key, col)
        for key in ("x_sum", "y_sum"):
            assert not after[key][:, col].any(), (key, col)
        assert after["eta"][col] == eta[i] and after["omega"][col] == omega[i]
        assert after["eta_sum"][col] == 0 and after["wpend"][col] == 0
        if attached:
            assert same_bits(after["K_valB"][:, col], h["K_val"][:, i]) and same_bits(after["KT_valB"][:, col], h["KT_val"][:, i])
    # a feed that lacks a per-LP vector, or lists more columns than the batch has, is refused before any launch
    bad = dict(feed, c=None)
    with pytest.raises(N.PdlpError):
        be.admit(cols, ids, eta, omega, **bad)
    with pytest.raises(N.PdlpError):
        be.admit(list(range(8)) + [0], [0] * 9, eta, omega, **feed)
    assert all(same_bits(v, after[k]) for k, v in state(be).items())


def retire_engine(B, W, dtype=torch.float32, factors=None):
    """a batch of B LPs 11 adaptive iterations in, averaged (x_avg and x_prev differ from x); ``factors``: "shared" -- the Ruiz
    scaling of the family's one K --, "per_lp" -- a matrix per LP (matrix_noise) with every LP's own factors"""
    f = family(B, seed=64, dtype=dtype, noise=0.2 if factors == "per_lp" else 0.0)
    K, kw = csr(f), {}
    if factors == "shared":
        K, scaling = tp.equilibrate_matrix(K, device=dev())
        kw = dict(d_col=scaling.d_col, d_row=scaling.d_row)
    elif factors == "per_lp":
        sv, stv, dc, dr, _ = tp.ruiz_precondition_batch(K, f.vals.to(dev()))
        kw = dict(K_values=sv, KT_values=stv, d_col=dc, d_row=dr)
    d = lambda v: v.to(dev())
    be = BatchEngine(K, f.m_ineq, d(f.C), d(f.Q), d(f.L), d(f.U), B, W=W, **kw)
    t = np.float32 if dtype == torch.float32 else np.float64
    eta = ((0.9 / norm2(f)) * np.linspace(0.7, 1.3, B)).astype(t)
    be.start(eta, np.linspace(0.5, 2.0, B).astype(t), d(f.X_opt).to(dtype) * 0.5, d(f.Y_opt).to(dtype) * 0.5)
    be.iterate(11, True, 0)
    be.average(True)
    return f, be


RETIRE_CASES = {
    # id: (B, W, dtype, which, factors, cols, ids); the result arrays have 6 columns.  Two groups: W = 16 with B = 32, W = 32 with 64
    "f32_w8_cur": (8, 8, torch.float32, N.CUR, None, [6, 2], [1, 4]),
    "w16_second_group_only": (32, 16, torch.float32, N.CUR, None, [20, 29], [1, 4]),        # group 0 leaves at once
    "w16_both_groups": (32, 16, torch.float32, N.CUR, None, [3, 20, 15], [5, 0, 2]),
    "w32_second_group_only": (64, 32, torch.float32, N.CUR, None, [40, 63], [4, 1]),
    "w32_both_groups": (64, 32, torch.float32, N.CUR, None, [5, 33, 62], [0, 3, 2]),
    "w8_avg": (8, 8, torch.float32, N.AVG, None, [6, 2], [1, 4]),
    "w8_prev": (8, 8, torch.float32, N.PREV, None, [0, 7], [5, 3]),
    "unscaled_shared_factors": (8, 8, torch.float32, N.CUR, "shared", [6, 2], [1, 4]),
    "unscaled_per_lp_matrices": (8, 8, torch.float32, N.CUR, "per_lp", [1, 5, 4], [2, 0, 3]),
    "f64_w16": (32, 16, torch.float64, N.CUR, None, [17, 4], [3, 1]),
    # an entry with a column outside [0, Bp) or an id outside [0, 6) is skipped: (-1, 0), (8, 2) and (3, 6) serve nobody
    "out_of_range_entries": (8, 8, torch.float32, N.CUR, None, [6, -1, 8, 2, 3], [1, 0, 2, 4, 6]),
}


@pytest.mark.parametrize("case", list(RETIRE_CASES), ids=list(RETIRE_CASES))
def test_retire_is_the_report_of_the_listed_columns(case):
    B, W, dtype, which, factors, cols, ids = RETIRE_CASES[case]
    unscaled = factors is not None
    f, be = retire_engine(B, W, dtype, factors)
    src_x, src_y = {N.CUR: (be.x, be.y), N.AVG: (be.x_avg, be.y_avg), N.PREV: (be.x_prev, be.y_prev)}[which]
    assert not torch.equal(be.x_avg[:, :B], be.x[:, :B]) and not torch.equal(be.x_prev[:, :B], be.x[:, :B])
    rc, act, sums = be.report(which, unscaled=unscaled, slot=1)
    rc, act = rc.clone(), act.clone()
    Nr, poison = 6, 7.5
    X, Y, RC, ACT = (torch.full((rows, Nr), poison, dtype=dtype, device=dev()) for rows in (f.n, f.m, f.n, f.m))
    be.out.fill_(poison)
    served = [(c, i) for c, i in zip(cols, ids) if 0 <= c < be.Bp and 0 <= i < Nr]
    assert len(served) >= 2 and len({c // W for c, _ in served}) == (2 if "both_groups" in case or case == "f64_w16" else 1)
    before = state(be)
    be.retire(cols, ids, X, Y, RC, ACT, which, unscaled=unscaled, slot=1)
    out = be.out.cpu().numpy()
    assert all(same_bits(v, before[k]) for k, v in state(be).items())             # nothing of the batch is written
    for col, i in served:
        assert torch.equal(X[:, i], src_x[:, col]) and torch.equal(Y[:, i], src_y[:, col])
        assert torch.equal(RC[:, i], rc[:, col]) and torch.equal(ACT[:, i], act[:, col])
        assert same_bits(out[1, col], sums[col])
    others = [i for i in range(Nr) if i not in [i for _, i in served]]
    for v in (X, Y, RC, ACT):
        assert (v[:, others] == poison).all()
    mask = np.ones(out.shape, bool)
    mask[1, [c for c, _ in served]] = False
    assert (out[mask] == poison).all()
    # without the optional arrays: the iterates and the sums only
    X2, Y2 = torch.full_like(X, poison), torch.full_like(Y, poison)
    be.retire(cols, ids, X2, Y2, None, None, which, unscaled=unscaled, slot=1)
    assert torch.equal(X2, X) and torch.equal(Y2, Y) and same_bits(be.out.cpu().numpy(), out)


def test_a_matrix_per_lp_streamed():
    f = family(24, seed=65, noise=0.2)
    sig = np.array([norm2(f, f.vals[:, b]) for b in range(24)])
    x0, y0 = uneven_start(f)
    plain, rp, _ = solve(f, sigma=sig, K_values=f.vals, x_init=x0, y_init=y0)
    streamed, rs, sched = solve(f, slots=8, sigma=sig, K_values=f.vals, x_init=x0, y_init=y0)
    assert plain[6] == ["Solved"] * 24
    assert_overlap(sched, streamed[3])
    assert_same_solve(plain, rp, streamed, rs)
    # the values on the host: only 8 columns of them are ever on the device
    peak = []
    for slots in (None, 8):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        rep = {}
        d = lambda v: v.to(dev())
        out = pdlp_algorithm_batch(csr(f), f.m_ineq, d(f.C), d(f.Q), d(f.L), d(f.U), dev(), report=rep, slots=slots, group_width=8,
                                   sigma=sig, K_values=f.vals if slots else d(f.vals), x_init=d(x0), y_init=d(y0))
        peak.append(torch.cuda.max_memory_allocated() - base)
        assert_same_solve(plain, rp, out, rep)
        del out, rep
    assert peak[1] < peak[0], peak


@pytest.mark.parametrize("precondition", [False, True], ids=["plain", "ruiz"])
def test_solve_lp_batch_streamed_end_to_end(precondition):
    B = 33
    f = family(B, seed=43)                   # (the family of test_width_32_float32_solves_like_solve_lp)
    prob = (f.C[:, 0], csr(f), f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0])
    sched = {}
    res = tp.solve_lp_batch(prob, f.C, f.Q, f.L, f.U, device=dev(), seed=0, slots=8, precondition=precondition, schedule=sched)
    assert res.status == ["Solved"] * B and len(res) == B
    assert tuple(res.x.shape) == (f.n, B) and tuple(res.y.shape) == (f.m, B) and tuple(res.reduced_costs.shape) == (f.n, B)
    assert (sched["admitted_at"] >= 0).all() and sched["admitted_at"].max() > 0
    for b in range(B):
        scale = 1 + abs(f.opt_obj[b]) + float((f.C[:, b].double() * f.X_opt[:, b].double()).abs().sum())      # (test_widths_solve_every_lp)
        assert abs(res.objective[b] - f.opt_obj[b]) <= 2e-3 * scale, b
        one = res[b]
        assert one.status == "Solved" and one.iterations == res.iterations[b] and torch.equal(one.x.view(-1), res.x[:, b])
        assert one.primal_residual == res.primal_residual[b]
    # the plain batch of the same call: the same numbers (W = 8 on both sides)
    ref = tp.solve_lp_batch(prob, f.C, f.Q, f.L, f.U, device=dev(), seed=0, group_width=8, precondition=precondition)
    assert torch.equal(res.x, ref.x) and torch.equal(res.y, ref.y) and list(res.kkt_passes) == list(ref.kkt_passes)
    assert same_bits(res.gap, ref.gap) and torch.equal(res.reduced_costs, ref.reduced_costs)


def test_time_limit_cuts_the_queue():
    f = family(40, seed=67)
    sig = norm2(f)
    x0 = (0.25 * f.X_opt).float()
    out, rep, sched = solve(f, slots=8, sigma=sig, time_limit=0.0, x_init=x0)
    late = sched["never_admitted"]
    assert list(late) == list(range(8, 40))                              # the clock ran out under the first columns
    assert out[6] == [TIME_LIMIT] * 40 and not out[3].any() and not out[5].any()
    assert torch.equal(out[0], x0.to(dev())) and not out[1].any()        # the start points come back
    assert (sched["admitted_at"][late] == -1).all() and (sched["admitted_at"][:8] == 0).all()
    # the same call without a clock: the report of a start point is the plain batch's
    ref, rr, _ = solve(f, sigma=sig, time_limit=0.0, x_init=x0)
    assert_same_solve(ref, rr, out, rep)
    # a clock that runs out somewhere in the family: whoever never ran says so
    out, rep, sched = solve(f, slots=8, sigma=sig, time_limit=0.05, x_init=x0)
    late = sched["never_admitted"]
    assert late.size >= 1 and all(out[6][i] == TIME_LIMIT for i in late) and not out[3][late].any()
    assert torch.equal(out[0][:, late], x0[:, late].to(dev()))
    assert all(s in (TIME_LIMIT, "Solved") for s in out[6])


def test_max_kkt_is_counted_per_lp_from_its_admission():
    f = family(24, seed=68)
    sig = norm2(f)
    x0, y0 = uneven_start(f)
    cap = 150                                             # inside a period: 3 checks x (40 + 3) = 129, then 21 iterations
    plain, rp, _ = solve(f, sigma=sig, x_init=x0, y_init=y0, max_kkt=cap)
    streamed, rs, sched = solve(f, slots=8, sigma=sig, x_init=x0, y_init=y0, max_kkt=cap)
    assert KKT_LIMIT in plain[6] and "Solved" in plain[6]
    assert all(j >= cap for j, s in zip(plain[5], plain[6]) if s == KKT_LIMIT)
    assert (sched["admitted_at"] % 40 == 0).all() and sched["admitted_at"].max() > 0
    assert_same_solve(plain, rp, streamed, rs)
