#!/usr/bin/env python3
"""The diagonal quadratic objective (solve_lp's quad_diag=) measured against the LP iteration of the SAME engine in one process.

    python tools/bench_quad_diag.py [n] [nnz_per_row] [tol] [f32|f64] [rate_iters] [rounds]

The problem is the bench LP of recipe "mixed" (a known optimal x*) with d drawn in [1/4, 2] on about 60 % of the variables and
c - d x* as the linear part: x* stays optimal, the optimum is opt_lp - 1/2 x*'D x*.
rate: HIP events around ``iterate(rate_iters, adaptive)`` and ``halpern_iterate(rate_iters)`` with the diagonal set and with it
switched off (``set_objective_diag(None)``), in alternating windows, `rounds` times each after one warm-up of both.
solve: ``run_pdlp`` of the QP with the adaptive step, primal weight on, to `tol` (TIME_LIMIT seconds, default 300; SOLVES=0 skips
it): iterations, seconds and the objective against the constructed optimum."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torchpdlp_amd as tp
from torchpdlp_amd.solver import estimate_sigma, run_pdlp

arg = lambda i, default, conv: conv(sys.argv[i]) if len(sys.argv) > i else default
n, k, tol = arg(1, 1_000_000, int), arg(2, 5, int), arg(3, 1e-4, float)
prec, rate_iters, rounds = arg(4, "f32", str), arg(5, 200, int), arg(6, 3, int)
if prec not in ("f32", "f64"):
    sys.exit("the quadratic term runs in f32 or f64")
dt = torch.float32 if prec == "f32" else torch.float64
dev = torch.device("cuda", 0)
t0 = time.time()
lp = tp.gen_lp(n, n, k, seed=0, device=dev, dtype=dt, recipe="mixed")
K = tp.CsrPair(lp.m, lp.n, lp.rowptr, lp.colidx, lp.val)
g = torch.Generator(device="cpu").manual_seed(1)
d = (torch.randint(1, 9, (n,), generator=g).to(dt) / 4 * (torch.rand(n, generator=g) >= 0.4).to(dt)).to(dev)
xs = lp.x_feas.to(dt)
c_q = lp.c - d * xs
opt = float(lp.opt_obj) - 0.5 * float((d.double() * xs.double() * xs.double()).sum())
eng = tp.PdlpEngine.from_full(K, c_q, lp.q, lp.l, lp.u, lp.m_ineq, quad_diag=d)
torch.cuda.synchronize()
print(f"{n} x {n}, {k} per row, {prec}: set up in {time.time() - t0:.1f} s, kernels={eng.kernels}, {int((d > 0).sum())} variables with d > 0",
      flush=True)
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
MODES = {"fixed": lambda: eng.iterate(rate_iters, False), "adaptive": lambda: eng.iterate(rate_iters, True),
         "halpern": lambda: eng.halpern_iterate(rate_iters)}
for mode, fn in MODES.items():
    ms = {"lp": [], "quad": []}
    for r in range(rounds + 1):                                  # (round 0: the warm-up of both)
        for name, diag in (("lp", None), ("quad", d)):
            eng.set_objective_diag(diag)
            eng.set_iterate(zeros(eng.nl), zeros(eng.ml))
            eng.set_step(eta, 1.0, 1.0, 0)
            t = timed(fn)
            if r:
                ms[name].append(t)
    for name, v in ms.items():
        print(f"RATE {mode:8s} {name:4s} ms/iteration: {' '.join(f'{t:.4f}' for t in v)}  -> {1000 / np.median(v):.1f} iterations/s (median)",
              flush=True)
    print(f"RESULT rate n={n} k={k} {prec} {mode}: quad_diag / LP time per iteration = {np.median(ms['quad']) / np.median(ms['lp']):.4f}", flush=True)

if os.environ.get("SOLVES", "1") != "0":
    limit, max_kkt = float(os.environ.get("TIME_LIMIT", "300")), int(os.environ.get("MAX_KKT", "400000"))
    eng.set_objective_diag(d)
    x, obj, it, nr, j, status, secs = run_pdlp(eng, max_kkt=max_kkt, tol=tol, verbose=False, primal_update=True, adaptive=True,
                                               time_limit=limit, sigma=sigma)
    print(f"RESULT solve n={n} k={k} tol={tol} {prec}: status={status} objective={obj:.6f} optimum={opt:.6f} "
          f"relative difference={abs(obj - opt) / (1 + abs(opt)):.3g} iterations={it} restarts={nr} kkt_passes={j} seconds={secs:.3f}", flush=True)
