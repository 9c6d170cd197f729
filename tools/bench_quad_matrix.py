#!/usr/bin/env python3
"""The sparse quadratic objective (solve_lp's quad_matrix=) measured against the LP iteration of the SAME engine in one process.

    python tools/bench_quad_matrix.py [--adaptive] [n] [nnz_per_row] [tol] [f32|f64] [rate_iters] [rounds]

The problem is the bench LP of recipe "mixed" (a known optimal x*) with Q = B'B, B n x n with two entries per row (multiples of 1/2
at random columns), and c - Q x* as the linear part: x* stays optimal, the optimum is opt_lp - 1/2 x*'Q x*.
rate: HIP events around ``iterate(rate_iters, False)`` with Q set and with it taken away (``set_objective_matrix(None)``), in
alternating windows, `rounds` times each after one warm-up of both; the same step size in both.  The expected extra is one CSR
product over nnz(Q) plus two vector streams of length n (c read, g written; x is in cache from the gather).
solve: ``run_pdlp`` of the QP with the fixed, linearised step, primal weight on, to `tol` (TIME_LIMIT seconds, default 300; SOLVES=0
skips it): iterations, seconds and the objective against the constructed optimum.
--adaptive: the adaptive step of the QP (``objective_iterate``, ``quad_step="adaptive"``) beside the fixed one -- two more windows in
every round of the rate (``iterate(rate_iters, True)`` of the LP and ``objective_iterate(rate_iters)`` of the QP, from the same start
and start step; the expected extra over the fixed QP iteration is the rule's one-workgroup kernel and, in the product with Q, two
more vector streams of length n: the old x and the old g) and the solve with both step rules in turn, SOLVE_ROUNDS (default 3) times each."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch
import torchpdlp_amd as tp
from torchpdlp_amd.rules import qp_eta
from torchpdlp_amd.solver import estimate_quad_norm, estimate_sigma, run_pdlp

adaptive = "--adaptive" in sys.argv
sys.argv = [a for a in sys.argv if a != "--adaptive"]
arg = lambda i, default, conv: conv(sys.argv[i]) if len(sys.argv) > i else default
n, k, tol = arg(1, 1_000_000, int), arg(2, 5, int), arg(3, 1e-4, float)
prec, rate_iters, rounds = arg(4, "f32", str), arg(5, 200, int), arg(6, 3, int)
if prec not in ("f32", "f64"):
    sys.exit("the quadratic term runs in f32 or f64")
dt = torch.float32 if prec == "f32" else torch.float64
npt = np.float32 if prec == "f32" else np.float64
dev = torch.device("cuda", 0)
t0 = time.time()
lp = tp.gen_lp(n, n, k, seed=0, device=dev, dtype=dt, recipe="mixed")
K = tp.CsrPair(lp.m, lp.n, lp.rowptr, lp.colidx, lp.val)
rng = np.random.default_rng(1)
rows = np.repeat(np.arange(n), 2)
B = sp.coo_matrix((rng.integers(-3, 4, 2 * n) / 2.0, (rows, rng.integers(0, n, 2 * n))), shape=(n, n)).tocsr()
Q = (B.T @ B).tocsr()
Q.eliminate_zeros()
Q.sort_indices()
Qp = tp.CsrPair.from_any(Q, device=dev, dtype=dt)
xs = lp.x_feas.to(dt)
xs_h = xs.double().cpu().numpy()
Qx = Q @ xs_h
c_q = lp.c - torch.from_numpy(Qx).to(device=dev, dtype=dt)
opt = float(lp.opt_obj) - 0.5 * float(xs_h @ Qx)
eng = tp.PdlpEngine.from_full(K, c_q, lp.q, lp.l, lp.u, lp.m_ineq, quad_matrix=Qp)
torch.cuda.synchronize()
print(f"{n} x {n}, {k} per row, {prec}: set up in {time.time() - t0:.1f} s, kernels={eng.kernels}, nnz(K)={K.nnz}, nnz(Q)={Qp.nnz}, "
      f"longest row of Q {int(np.diff(Q.indptr).max())}", flush=True)
sigma = estimate_sigma(eng, None, 100, 0)
L = estimate_quad_norm(eng, None, 100, 0)
eta = float(qp_eta(sigma, L, 1.0, npt))
print(f"||K|| ~ {sigma:.4f}, ||Q|| ~ {L:.4f}, eta = {eta:.6f} (the LP's: {0.9 / sigma:.6f})", flush=True)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.synchronize()
    e0.record(eng.stream)
    fn()
    e1.record(eng.stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / rate_iters


zeros = lambda ln: torch.zeros(ln, dtype=dt, device=dev)
windows = [("lp", None, "fixed"), ("qmat", Qp, "fixed")] + ([("lp", None, "adaptive"), ("qmat", Qp, "adaptive")] if adaptive else [])
ms = {w: [] for w in windows}
for r in range(rounds + 1):                                  # (round 0: the warm-up of all)
    for w in windows:
        name, mat, step = w
        eng.set_objective_matrix(mat)
        eng.set_iterate(zeros(eng.nl), zeros(eng.ml))
        eng.set_step(eta, 1.0, 1.0, 0)
        if step == "fixed":
            t = timed(lambda: eng.iterate(rate_iters, False))
        elif mat is None:
            t = timed(lambda: eng.iterate(rate_iters, True))
        else:
            t = timed(lambda: eng.objective_iterate(rate_iters))
        if r:
            ms[w].append(t)
for (name, _, step), v in ms.items():
    print(f"RATE {step} {name:4s} ms/iteration: {' '.join(f'{t:.4f}' for t in v)}  -> {1000 / np.median(v):.1f} iterations/s (median)", flush=True)
ms = {(name, step): v for (name, _, step), v in ms.items()}
if adaptive:
    qa, qf, la = (np.median(ms[k]) for k in (("qmat", "adaptive"), ("qmat", "fixed"), ("lp", "adaptive")))
    print(f"RESULT rate n={n} k={k} {prec} adaptive: quad_matrix adaptive / fixed time per iteration = {qa / qf:.4f} ({qa - qf:+.4f} ms); "
          f"against the adaptive LP iteration = {qa / la:.4f} ({qa - la:+.4f} ms)", flush=True)
ms = {name: v for (name, step), v in ms.items() if step == "fixed"}
print(f"RESULT rate n={n} k={k} {prec} fixed: quad_matrix / LP time per iteration = {np.median(ms['qmat']) / np.median(ms['lp']):.4f} "
      f"(+{np.median(ms['qmat']) - np.median(ms['lp']):.4f} ms)", flush=True)

if os.environ.get("SOLVES", "1") != "0":
    limit, max_kkt = float(os.environ.get("TIME_LIMIT", "300")), int(os.environ.get("MAX_KKT", "400000"))
    eng.set_objective_matrix(Qp)
    # --adaptive: the two step rules solve in turn, SOLVE_ROUNDS times -- the first solve of a process also loads the kernels of
    # the restart checks, and it is the later rounds that compare
    for r in range(int(os.environ.get("SOLVE_ROUNDS", "3")) if adaptive else 1):
        for step in ("fixed", "adaptive") if adaptive else ("fixed",):
            x, obj, it, nr, j, status, secs = run_pdlp(eng, max_kkt=max_kkt, tol=tol, verbose=False, primal_update=True, time_limit=limit,
                                                       sigma=sigma, quad_norm=L, quad_step=step)
            tag = f" quad_step={step} round={r}" if adaptive else ""
            print(f"RESULT solve n={n} k={k} tol={tol} {prec}{tag}: status={status} objective={obj:.6f} optimum={opt:.6f} "
                  f"relative difference={abs(obj - opt) / (1 + abs(opt)):.3g} iterations={it} restarts={nr} kkt_passes={j} seconds={secs:.3f}"
                  + (f" (last eta {eng.scalars()['eta']:.6f})" if adaptive else ""), flush=True)
