"""Batched solves on the MI355X (pdlp_batch_*, torchpdlp_amd/batch.py): every LP of a batch against the oracle and against the
single-LP solver, bit-identity across batches, frozen LPs, broadcast vectors, Ruiz, the limits and an MPS family."""
import os

import numpy as np
import pytest
import torch

import torchpdlp_amd as tp
from torchpdlp_amd.batch import pdlp_algorithm_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    return torch.device("cuda", 0)


def family(B, seed=3, n=300, m=240, dtype=torch.float32):
    return tp.gen_lp_family(n, m, 4, B, seed=seed, dtype=dtype)


def csr(f, dtype=None):
    return tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val if dtype is None else f.val.to(dtype)).to(dev())


def oracle_lp(f, b, dtype):
    from oracle import oracle as orc
    return orc.OracleLP(f.m, f.n, f.m_ineq, f.rowptr.numpy(), f.colidx.numpy(), f.val.numpy(), f.C[:, b].numpy(), f.Q[:, b].numpy(),
                        f.L[:, b].numpy(), f.U[:, b].numpy(), dtype=dtype)


def norm2(f):
    """||K||_2 of the family's matrix (the power iteration's target), so that every solver here starts from the same sigma"""
    K = torch.sparse_csr_tensor(f.rowptr, f.colidx.long(), f.val.double(), (f.m, f.n)).to_dense().numpy()
    return float(np.linalg.norm(K, 2))


def run(f, sigma=None, cols=None, **kw):
    sigma = norm2(f) if sigma is None else sigma
    cols = list(range(f.B)) if cols is None else cols
    d = lambda v: v[:, cols].to(dev())
    return pdlp_algorithm_batch(csr(f), f.m_ineq, d(f.C), d(f.Q), d(f.L), d(f.U), dev(), sigma=sigma, **kw)


def golden_family(B=5, dtype=np.float32):
    """the 400 x 300 golden LP (solve_trace.npz, its b0) and B-1 more columns: c perturbed, q = K xh - s with xh inside the bounds
    and s >= 0 on the inequality rows (every column stays feasible); column 0 is the golden LP itself"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "solve_trace.npz"))
    a = lambda k: g[f"mixed_400x300/{k}"]
    m, n, mi = int(a("m")), int(a("n")), int(a("m_ineq"))
    rp, ci, va = a("rowptr"), a("colidx"), a("val").astype(dtype)
    K = np.zeros((m, n))
    for i in range(m):
        K[i, ci[rp[i]:rp[i + 1]]] += va[rp[i]:rp[i + 1]]
    rng = np.random.default_rng(11)
    l, u = a("l").astype(dtype), a("u").astype(dtype)
    C, Q = [a("c").astype(dtype)], [a("q").astype(dtype)]
    for _ in range(1, B):
        C.append((a("c") * (1 + 0.1 * rng.standard_normal(n))).astype(dtype))
        xh = np.clip(rng.uniform(-1, 1, n), l, u)
        s = np.where(np.arange(m) < mi, rng.uniform(0, 1, m), 0.0)
        Q.append((K @ xh - s).astype(dtype))
    return dict(m=m, n=n, m_ineq=mi, rp=rp, ci=ci, va=va, C=np.stack(C, 1), Q=np.stack(Q, 1), l=l, u=u, b0=a("fixed_nopw/b0"))


def golden_oracle(G, b, dtype):
    from oracle import oracle as orc
    return orc.OracleLP(G["m"], G["n"], G["m_ineq"], G["rp"], G["ci"], G["va"], G["C"][:, b], G["Q"][:, b], G["l"], G["u"], dtype=dtype)


def golden_batch(G, dtype, **kw):
    t = lambda v, dt=dtype: torch.tensor(np.asarray(v), dtype=dt, device=dev())
    K = tp.CsrPair(G["m"], G["n"], t(G["rp"], torch.int32), t(G["ci"], torch.int32), t(G["va"]))
    traces = [dict(kkt=[], omega=[], restarts=[]) for _ in range(G["C"].shape[1])]
    out = pdlp_algorithm_batch(K, G["m_ineq"], t(G["C"]), t(G["Q"]), t(G["l"]), t(G["u"]), dev(), b0=t(G["b0"], torch.float32),
                               traces=traces, **kw)
    return out, traces, K, t


def test_trace_against_the_oracle_float32_fixed():
    from oracle import oracle as orc
    G = golden_family()
    out, traces, _, _ = golden_batch(G, torch.float32)          # B = 5: W = 8, three padding columns
    for b in range(5):
        *_, tr = orc.pdlp_algorithm(golden_oracle(G, b, np.float32), b0=G["b0"])
        assert [tuple(r) for r in traces[b]["restarts"][:5]] == [tuple(r) for r in tr["restarts"][:5]], b
        np.testing.assert_allclose(traces[b]["kkt"][:10], tr["kkt"][:10], rtol=5e-4)


def test_trace_against_the_oracle_float32_adaptive_primal_weight():
    from oracle import oracle as orc
    G = golden_family()
    out, traces, _, _ = golden_batch(G, torch.float32, adaptive=True, primal_update=True)
    for b in range(5):
        *_, tr = orc.pdlp_algorithm(golden_oracle(G, b, np.float32), b0=G["b0"], adaptive=True, primal_update=True)
        assert [tuple(r) for r in traces[b]["restarts"][:1]] == [tuple(r) for r in tr["restarts"][:1]], b
        np.testing.assert_allclose(traces[b]["kkt"][:4], tr["kkt"][:4], rtol=5e-2)
        np.testing.assert_allclose(traces[b]["omega"][:1], tr["omega"][:1], rtol=5e-2)


def test_float64_matches_the_oracle_and_the_single_lp_solver():
    from oracle import oracle as orc
    G = golden_family(dtype=np.float64)
    (X, Y, obj, k, n, j, st, _), traces, K, t = golden_batch(G, torch.float64)
    for b in range(5):
        *_, tr = orc.pdlp_algorithm(golden_oracle(G, b, np.float64), b0=G["b0"])
        assert [tuple(r) for r in traces[b]["restarts"][:10]] == [tuple(r) for r in tr["restarts"][:10]], b
        np.testing.assert_allclose(traces[b]["kkt"][:10], tr["kkt"][:10], rtol=1e-9)
        d = lambda v: t(v[:, b] if v.ndim == 2 else v)
        _, _, ks, ns, js, sts, _ = tp.pdlp_algorithm(K, G["m_ineq"], d(G["C"]), d(G["Q"]), d(G["l"]), d(G["u"]), dev(), verbose=False,
                                                     b0=t(G["b0"], torch.float32))
        assert (int(k[b]), int(n[b]), int(j[b]), st[b]) == (ks, ns, js, sts), b


def test_an_lp_does_not_depend_on_its_batch():
    f, g = family(8, seed=6), family(8, seed=7)
    a = run(f, group_width=16)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    mix = lambda v, w: torch.cat([v[:, perm], w[:, :6]], dim=1)
    h = type(f)(f.m, f.n, f.m_ineq, f.rowptr, f.colidx, f.val, mix(f.C, g.C), mix(f.Q, g.Q), mix(f.L, g.L), mix(f.U, g.U),
                f.X_opt, f.Y_opt, f.opt_obj)
    b_ = run(h, group_width=16)
    for pos, i in enumerate(perm):
        assert torch.equal(a[0][:, i], b_[0][:, pos]) and torch.equal(a[1][:, i], b_[1][:, pos]), i
        assert (a[3][i], a[4][i], a[5][i]) == (b_[3][pos], b_[4][pos], b_[5][pos]), i


def dense(f):
    return torch.sparse_csr_tensor(f.rowptr, f.colidx.long(), f.val.double(), (f.m, f.n)).to_dense().numpy()


def feasible(K, f, x, b):
    q = f.Q[:, b].double().numpy()
    r = K @ x - q
    viol = np.concatenate([np.minimum(r[:f.m_ineq], 0), r[f.m_ineq:]])
    return np.linalg.norm(viol) <= 1.5e-4 * (1 + np.linalg.norm(q))


@pytest.mark.parametrize("B", [1, 8, 9, 33, 100])
def test_widths_solve_every_lp(B):
    """one group, several gridDim.y groups and padding (float32: W = 8 / 16 / 32)"""
    f = family(B, seed=10 + B)
    res = tp.solve_lp_batch((f.C[:, 0], csr(f), f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0]), f.C, f.Q, f.L, f.U, device=dev(), seed=0)
    assert res.status == ["Solved"] * B
    K = dense(f)
    for b in range(B):
        # 2e-3 relative to the size of the objective's terms: the reference's signed-gap test at tol 1e-4 bounds the error by
        # tol (1 + |p| + |d|), which on an LP whose optimum is near 0 (terms of size 10, sum 0.01) is far more than 2e-3 |opt|
        scale = 1 + abs(f.opt_obj[b]) + float((f.C[:, b].double() * f.X_opt[:, b].double()).abs().sum())
        assert abs(res.objective[b] - f.opt_obj[b]) <= 2e-3 * scale, b
        assert feasible(K, f, res.x[:, b].double().cpu().numpy(), b), b
        assert res[b].status == "Solved"


def test_width_32_float32_solves_like_solve_lp():
    """float32, B = 33: W = 32, two groups (31 padding columns); each LP against solve_lp on that LP alone"""
    f = family(33, seed=43)
    res = tp.solve_lp_batch((f.C[:, 0], csr(f), f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0]), f.C, f.Q, f.L, f.U, device=dev(), seed=0)
    assert res.status == ["Solved"] * 33
    K = dense(f)
    for b in range(33):
        one = tp.solve_lp((f.C[:, b].to(dev()), csr(f), f.Q[:, b].to(dev()), f.m_ineq, f.L[:, b].to(dev()), f.U[:, b].to(dev())),
                          device=dev(), seed=0)
        assert one.status == "Solved"
        assert abs(res.objective[b] - one.objective) <= 2e-3 * (1 + abs(one.objective)), b
        assert feasible(K, f, res.x[:, b].double().cpu().numpy(), b), b


def test_frozen_lp_is_untouched_by_the_rest():
    """LP 2 starts at its optimum: solved at its first restart (k = 40); the others start at 0 and need many restarts"""
    f = family(8, seed=21)
    x0 = torch.zeros(f.n, 8)
    y0 = torch.zeros(f.m, 8)
    x0[:, 2], y0[:, 2] = f.X_opt[:, 2], f.Y_opt[:, 2]
    a = run(f, x_init=x0.to(dev()), y_init=y0.to(dev()))
    assert a[6][2] == "Solved" and (a[3][2], a[4][2]) == (40, 1)
    assert a[6] == ["Solved"] * 8 and min(a[4][b] for b in range(8) if b != 2) >= 2
    alone = run(f, cols=[2], group_width=8, x_init=x0[:, 2:3].to(dev()), y_init=y0[:, 2:3].to(dev()))
    # bit-identical to the batch in which it is alone: its column was never written after it froze
    assert torch.equal(a[0][:, 2], alone[0][:, 0]) and torch.equal(a[1][:, 2], alone[1][:, 0])
    assert (a[3][2], a[4][2], a[5][2], a[6][2]) == (alone[3][0], alone[4][0], alone[5][0], alone[6][0])


def test_broadcast_vectors_equal_materialised_columns():
    f = family(6, seed=30)
    d = lambda v: v.to(dev())
    shared = pdlp_algorithm_batch(csr(f), f.m_ineq, d(f.C[:, 0]), d(f.Q), d(f.L[:, 0]), d(f.U[:, 0]), dev(), sigma=norm2(f))
    rep = lambda v: d(v[:, :1].repeat(1, 6))
    full = pdlp_algorithm_batch(csr(f), f.m_ineq, rep(f.C), d(f.Q), rep(f.L), rep(f.U), dev(), sigma=norm2(f))
    assert torch.equal(shared[0], full[0]) and torch.equal(shared[1], full[1])
    assert list(shared[3]) == list(full[3]) and shared[6] == full[6]


def test_ruiz_matches_solve_lp():
    f = family(8, seed=40)
    prob = (f.C[:, 0], csr(f), f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0])
    res = tp.solve_lp_batch(prob, f.C, f.Q, f.L, f.U, device=dev(), precondition=True, seed=0)
    for b in range(8):
        one = tp.solve_lp((f.C[:, b].to(dev()), csr(f), f.Q[:, b].to(dev()), f.m_ineq, f.L[:, b].to(dev()), f.U[:, b].to(dev())),
                          device=dev(), precondition=True, seed=0)
        assert res.status[b] == one.status
        assert abs(res.objective[b] - one.objective) <= 2e-3 * (1 + abs(one.objective)), b
    # x and y come back un-scaled: x near solve_lp's (un-scaled) x, and y the scaled dual times D_row
    K = dense(f)
    for b in range(8):
        x, y = res.x[:, b].double().cpu().numpy(), res.y[:, b].double().cpu().numpy()
        c, q, l, u = (v[:, b].double().numpy() for v in (f.C, f.Q, f.L, f.U))
        one = tp.solve_lp((f.C[:, b].to(dev()), csr(f), f.Q[:, b].to(dev()), f.m_ineq, f.L[:, b].to(dev()), f.U[:, b].to(dev())),
                          device=dev(), precondition=True, seed=0)
        xo = one.x.view(-1).double().cpu().numpy()
        assert np.linalg.norm(x - xo) <= 2e-2 * (1 + np.linalg.norm(xo)), b
        assert (y[:f.m_ineq] >= 0).all(), b
    # y = D_row y_s: the scaled dual of the same batch, multiplied out on the host
    Ks, scaling = tp.equilibrate_matrix(csr(f), device=dev())
    dp = (scaling.d_col, scaling.d_row)
    Dc, Dr = dp[0].view(-1, 1), dp[1].view(-1, 1)
    Xs, Ys, *_ = pdlp_algorithm_batch(Ks, f.m_ineq, f.C.to(dev()) * Dc, f.Q.to(dev()) * Dr, f.L.to(dev()) / Dc, f.U.to(dev()) / Dc,
                                      dev(), precondition=True, data_precond=dp, seed=0)
    assert torch.equal(res.x, Dc * Xs) and torch.equal(res.y, Dr * Ys)


def test_limits():
    f = family(8, seed=50)
    a = run(f)
    cap = int(np.median(a[5]))
    c = run(f, max_kkt=cap)
    for b in range(8):
        want = "Solved" if a[5][b] <= cap else "Unsolved (KKT passes limit exceeded)"
        assert c[6][b] == want, (b, a[5][b], cap, c[6][b])
        assert c[5][b] <= cap + 5
    t = run(f, time_limit=0.0)
    assert t[6] == ["Unsolved (Time limit exceeded)"] * 8


def test_mps_family_against_highs():
    scipy_opt = pytest.importorskip("scipy.optimize")
    path = os.path.join(ROOT, "tests", "golden", "mps", "afiro.mps")
    c, K, q, m_ineq, l, u = tp.mps_to_standard_form(path, device="cpu")
    c, q, l, u = (v.reshape(-1) for v in (c, q, l, u))
    Kd = K.to_dense().double().numpy() if hasattr(K, "to_dense") else None
    if Kd is None:
        Kd = torch.sparse_csr_tensor(K.rowptr, K.colidx.long(), K.val.double(), (K.m, K.n)).to_dense().numpy()
    rng = np.random.default_rng(0)
    Q = np.stack([q.double().numpy() * (1 + 0.02 * rng.standard_normal(q.shape[0])) for _ in range(8)], axis=1)
    res = tp.solve_lp_batch(path, q=torch.from_numpy(Q).float(), device=dev(), seed=0)
    for b in range(8):
        bounds = list(zip(*(np.where(np.isinf(v), None, v) for v in (l.double().numpy(), u.double().numpy()))))
        h = scipy_opt.linprog(c.double().numpy(), A_ub=-Kd[:m_ineq], b_ub=-Q[:m_ineq, b], A_eq=Kd[m_ineq:], b_eq=Q[m_ineq:, b],
                              bounds=bounds, method="highs")
        if h.status != 0:
            continue
        assert res.status[b] == "Solved", b
        assert abs(res.objective[b] - h.fun) <= 2e-3 * (1 + abs(h.fun)), (b, res.objective[b], h.fun)
