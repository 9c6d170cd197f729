#!/usr/bin/env python3
"""The Halpern solve mode (solve_lp's halpern=True) measured against averaged PDHG on the bench LP, on ONE engine in one process.

    python tools/bench_halpern.py [n] [nnz_per_row] [tol] [ruiz 0/1] [f32|f64] [rate_iters] [rounds] [--halpern-restart fixed_point]
    python tools/bench_halpern.py --mps FILE tol f32|f64 [--halpern-restart fixed_point]      (solves only, on the LP of an MPS file)

rate: HIP events around ``iterate(rate_iters, adaptive=False)`` and ``halpern_iterate(rate_iters)``, alternating, `rounds` times each
after one warm-up of both (no restart check inside: the iteration alone).
solves: ``run_pdlp`` with the adaptive step (the configuration of the README's headline), with the fixed step, and with
``halpern=True``, primal weight on, seed 0, the same power-iteration estimate: iterations, restarts, KKT passes and seconds each
(TIME_LIMIT seconds per solve, default 300; MAX_KKT passes, default 400000).  SOLVES=0 skips them.
--halpern-restart fixed_point: one more solve, ``halpern=True, halpern_restart="fixed_point"`` (the restart checks look at the fixed-point
residual instead of the candidate's KKT error), and the cost of a restart check under both rules: ``PdhgDriver.check_seconds`` over the
first CHECKS checks (default 10) of a run from zero on the same engine, per check -- the checks that kept going and the checks that
restarted apart (a check that restarts also does the restart's work: primal weight, mark, the KKT pass of the termination test)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torchpdlp_amd as tp
from torchpdlp_amd.solver import PdhgDriver, estimate_sigma, run_pdlp

fixed_point = False
if "--halpern-restart" in sys.argv:
    at = sys.argv.index("--halpern-restart")
    if sys.argv[at + 1:at + 2] not in (["kkt"], ["fixed_point"]):
        sys.exit("--halpern-restart kkt|fixed_point")
    fixed_point = sys.argv[at + 1] == "fixed_point"
    del sys.argv[at:at + 2]
mps = None
if "--mps" in sys.argv:
    at = sys.argv.index("--mps")
    mps = sys.argv[at + 1]
    del sys.argv[at:at + 2]
    sys.argv[1:1] = ["0", "0"]                        # (no generated shape)
    sys.argv[4:4] = ["0"]                             # (no Ruiz)
arg = lambda i, default, conv: conv(sys.argv[i]) if len(sys.argv) > i else default
n, k, tol = arg(1, 1_000_000, int), arg(2, 5, int), arg(3, 1e-4, float)
ruiz, prec, rate_iters, rounds = arg(4, "0", str) == "1", arg(5, "f32", str), arg(6, 200, int), arg(7, 3, int)
if prec not in ("f32", "f64"):
    sys.exit("the Halpern mode runs in f32 or f64")
dt = torch.float32 if prec == "f32" else torch.float64
dev = torch.device("cuda", 0)
t0 = time.time()
if mps:
    c, K, q, m_ineq, l, u = tp.mps_to_standard_form(mps, device=dev, dtype=dt)
    n, k = int(K.n), os.path.basename(mps)
else:
    lp = tp.gen_lp(n, n, k, seed=0, device=dev, dtype=dt)
    K = tp.CsrPair(lp.m, lp.n, lp.rowptr, lp.colidx, lp.val)
    c, q, l, u, m_ineq = lp.c, lp.q, lp.l, lp.u, lp.m_ineq
dcol = drow = None
if ruiz:
    K, c, q, l, u, dp, _ = tp.ruiz_precondition(c, K, q, l, u, device=dev)
    dcol, drow = dp[0], dp[1]
eng = tp.PdlpEngine.from_full(K, c, q, l, u, m_ineq, d_col=dcol, d_row=drow)
torch.cuda.synchronize()
print(f"{K.m} x {K.n}, {k} per row, {prec}, ruiz={ruiz}: set up in {time.time() - t0:.1f} s, kernels={eng.kernels}", flush=True)
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
if not mps:
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
    methods = [("adaptive", dict(adaptive=True)), ("fixed", dict()), ("halpern", dict(halpern=True))]
    if fixed_point:
        methods.append(("halpern_fixed_point", dict(halpern=True, halpern_restart="fixed_point")))
    for name, kw in methods:
        x, obj, it, nr, j, status, secs = run_pdlp(eng, max_kkt=max_kkt, tol=tol, verbose=False, precondition=ruiz, primal_update=True,
                                                   time_limit=limit, sigma=sigma, **kw)
        print(f"RESULT solve n={n} k={k} tol={tol} ruiz={ruiz} {prec} method={name}: status={status} objective={obj:.6f} iterations={it} "
              f"restarts={nr} kkt_passes={j} seconds={secs:.3f}", flush=True)

if fixed_point:
    checks = int(os.environ.get("CHECKS", "10"))
    for rule in ("kkt", "fixed_point"):
        drv = PdhgDriver(eng, 40, primal_update=True, precondition=ruiz, tol=tol, halpern=True, halpern_restart=rule)
        drv.start(sigma)
        drv.check_seconds = 0.0
        kept, restarted = [], []
        while drv.checks < checks and not drv.solved:
            before, n0, c0 = drv.check_seconds, drv.n, drv.checks
            drv.advance(40)
            if drv.checks > c0:
                (restarted if drv.n > n0 else kept).append(1000 * (drv.check_seconds - before))
        med = lambda v: f"{np.median(v):.4f}" if v else "-"
        print(f"RESULT check n={n} k={k} {prec} ruiz={ruiz} halpern_restart={rule}: checks={drv.checks} restarts={drv.n} "
              f"ms per check without a restart (median of {len(kept)}) = {med(kept)}; with a restart (median of {len(restarted)}) = {med(restarted)}",
              flush=True)
