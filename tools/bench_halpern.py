#!/usr/bin/env python3
"""The Halpern solve mode (solve_lp's halpern=True) measured against averaged PDHG on the bench LP, on ONE engine in one process.

    python tools/bench_halpern.py [n] [nnz_per_row] [tol] [ruiz 0/1] [f32|f64] [rate_iters] [rounds]

rate: HIP events around ``iterate(rate_iters, adaptive=False)`` and ``halpern_iterate(rate_iters)``, alternating, `rounds` times each
after one warm-up of both (no restart check inside: the iteration alone).
solves: ``run_pdlp`` with the adaptive step (the configuration of the README's headline), with the fixed step, and with
``halpern=True``, primal weight on, seed 0, the same power-iteration estimate: iterations, restarts, KKT passes and seconds each
(TIME_LIMIT seconds per solve, default 300; MAX_KKT passes, default 400000).  SOLVES=0 skips them."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torchpdlp_amd as tp
from torchpdlp_amd.solver import estimate_sigma, run_pdlp

arg = lambda i, default, conv: conv(sys.argv[i]) if len(sys.argv) > i else default
n, k, tol = arg(1, 1_000_000, int), arg(2, 5, int), arg(3, 1e-4, float)
ruiz, prec, rate_iters, rounds = arg(4, "0", str) == "1", arg(5, "f32", str), arg(6, 200, int), arg(7, 3, int)
if prec not in ("f32", "f64"):
    sys.exit("the Halpern mode runs in f32 or f64")
dt = torch.float32 if prec == "f32" else torch.float64
dev = torch.device("cuda", 0)
t0 = time.time()
lp = tp.gen_lp(n, n, k, seed=0, device=dev, dtype=dt)
K = tp.CsrPair(lp.m, lp.n, lp.rowptr, lp.colidx, lp.val)
c, q, l, u = lp.c, lp.q, lp.l, lp.u
dcol = drow = None
if ruiz:
    K, c, q, l, u, dp, _ = tp.ruiz_precondition(c, K, q, l, u, device=dev)
    dcol, drow = dp[0], dp[1]
eng = tp.PdlpEngine.from_full(K, c, q, l, u, lp.m_ineq, d_col=dcol, d_row=drow)
torch.cuda.synchronize()
print(f"{n} x {n}, {k} per row, {prec}, ruiz={ruiz}: set up in {time.time() - t0:.1f} s, kernels={eng.kernels}", flush=True)
sigma = estimate_sigma(eng, None, 100, 0)
eta = 0.9 / sigma


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.synchronize()
    e0.record(eng.stream)
    fn()
    e1.record(eng.stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / rate_iters


zeros = lambda ln: torch.zeros(ln, dtype=dt, device=dev)
eng.set_iterate(zeros(eng.nl), zeros(eng.ml))
eng.set_step(eta, 1.0, 1.0, 0)
pdhg, halp = lambda: eng.iterate(rate_iters, False), lambda: eng.halpern_iterate(rate_iters)
timed(pdhg), timed(halp)                                    # warm-up of both
ms = {"pdhg": [], "halpern": []}
for _ in range(rounds):
    ms["pdhg"].append(timed(pdhg))
    ms["halpern"].append(timed(halp))
for name, v in ms.items():
    print(f"RATE {name:8s} ms/iteration: {' '.join(f'{t:.4f}' for t in v)}  -> {1000 / np.median(v):.1f} iterations/s (median)", flush=True)
print(f"RESULT rate n={n} k={k} {prec}: halpern / fixed-step PDHG time per iteration = {np.median(ms['halpern']) / np.median(ms['pdhg']):.4f}",
      flush=True)

if os.environ.get("SOLVES", "1") != "0":
    limit, max_kkt = float(os.environ.get("TIME_LIMIT", "300")), int(os.environ.get("MAX_KKT", "400000"))
    for name, kw in (("adaptive", dict(adaptive=True)), ("fixed", dict()), ("halpern", dict(halpern=True))):
        x, obj, it, nr, j, status, secs = run_pdlp(eng, max_kkt=max_kkt, tol=tol, verbose=False, precondition=ruiz, primal_update=True,
                                                   time_limit=limit, sigma=sigma, **kw)
        print(f"RESULT solve n={n} k={k} tol={tol} ruiz={ruiz} {prec} method={name}: status={status} objective={obj:.6f} iterations={it} "
              f"restarts={nr} kkt_passes={j} seconds={secs:.3f}", flush=True)
