#!/usr/bin/env python3
"""Two-sided rows (solve_lp's q_upper) measured against the split form -- every two-sided row entered twice, as the MPS reader does
-- on a synthetic LP whose inequality rows ALL have a finite q_upper, one engine each in one process.

    python tools/bench_ranged_rows.py [n] [nnz_per_row] [tol] [f32|f64] [rate_iters] [rounds]

The LP: the bench LP (``gen_lp``, recipe "box": ``K x_feas`` strictly above ``q`` on the inequality rows) with
``q_upper = K x_feas + (K x_feas - q) / 2 + 0.1`` there, so ``x_feas`` is strictly inside both sides.
rate: HIP events around ``iterate(rate_iters, adaptive=False)`` on the native engine and on the split engine, alternating, `rounds`
times each after one warm-up of both (no restart check inside); the same for the Halpern iteration.
cost of RANGED where it is not needed: on the NATIVE engine, all-infinite q_upper (the RANGED functors) against no q_upper (the plain
ones), alternating windows of the same length.
solves: ``run_pdlp`` to `tol` with the adaptive step and the primal weight, seed 0, each form with its own power-iteration estimate:
iterations, restarts, KKT passes and seconds, after a warm-up of two restart periods of each form (TIME_LIMIT seconds per solve,
default 300; MAX_KKT, default 400000).  SOLVES=0 skips them."""
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
    sys.exit("two-sided rows run in f32 or f64")
dt = torch.float32 if prec == "f32" else torch.float64
dev = torch.device("cuda", 0)
t0 = time.time()
lp = tp.gen_lp(n, n, k, seed=0, device=dev, dtype=dt)
m, mi = lp.m, lp.m_ineq
K = tp.CsrPair(m, lp.n, lp.rowptr, lp.colidx, lp.val)
native = tp.PdlpEngine.from_full(K, lp.c, lp.q, lp.l, lp.u, mi)
kx = native.spmv(lp.x_feas)
q_upper = torch.full((m,), float("inf"), dtype=dt, device=dev)
q_upper[:mi] = kx[:mi] + 0.5 * (kx[:mi] - lp.q[:mi]).clamp_min(0) + 0.1
# the split twin: row i < m_ineq becomes rows 2i (as it is) and 2i + 1 (negated, right-hand side -q_upper_i); k entries in every row
col, val = lp.colidx.view(m, k), lp.val.view(m, k)
sign = torch.tensor([1.0, -1.0], dtype=dt, device=dev).repeat(mi).view(-1, 1)
col2 = torch.cat([col[:mi].repeat_interleave(2, dim=0), col[mi:]]).reshape(-1).contiguous()
val2 = torch.cat([val[:mi].repeat_interleave(2, dim=0) * sign, val[mi:]]).reshape(-1).contiguous()
q2 = torch.cat([torch.stack([lp.q[:mi], -q_upper[:mi]], dim=1).reshape(-1), lp.q[mi:]])
m2 = m + mi
K2 = tp.CsrPair(m2, lp.n, torch.arange(0, (m2 + 1) * k, k, dtype=torch.int64, device=dev), col2, val2)
split = tp.PdlpEngine.from_full(K2, lp.c, q2, lp.l, lp.u, 2 * mi)
del col2, val2, sign
torch.cuda.synchronize()
print(f"{n} x {n}, {k} per row, {prec}: {mi} two-sided rows; native {m} rows {K.nnz} non-zeros kernels={native.kernels}; "
      f"split {m2} rows {K2.nnz} non-zeros kernels={split.kernels}; set up in {time.time() - t0:.1f} s", flush=True)
sig = {"native": estimate_sigma(native, None, 100, 0), "split": estimate_sigma(split, None, 100, 0)}
engines = {"native": native, "split": split}


def timed(eng, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.synchronize()
    e0.record(eng.stream)
    fn()
    e1.record(eng.stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / rate_iters


def windows(label, runs):
    """runs: {name: (engine, callable)} timed in alternating windows after one warm-up of each"""
    for eng, fn in runs.values():
        timed(eng, fn)
    ms = {name: [] for name in runs}
    for _ in range(rounds):
        for name, (eng, fn) in runs.items():
            ms[name].append(timed(eng, fn))
    for name, v in ms.items():
        print(f"RATE {label} {name:8s} ms/iteration: {' '.join(f'{t:.4f}' for t in v)}  -> {1000 / np.median(v):.1f} iterations/s (median)",
              flush=True)
    return {name: float(np.median(v)) for name, v in ms.items()}


zeros = lambda ln: torch.zeros(ln, dtype=dt, device=dev)
native.set_row_upper(q_upper)
for name, eng in engines.items():
    eng.set_iterate(zeros(eng.nl), zeros(eng.ml))
    eng.set_step(0.9 / sig[name], 1.0, 1.0, 0)
med = windows("pdhg", {name: (eng, (lambda e=eng: e.iterate(rate_iters, False))) for name, eng in engines.items()})
print(f"RESULT rate n={n} k={k} {prec} fixed-step PDHG: native / split time per iteration = {med['native'] / med['split']:.4f}", flush=True)
med = windows("halpern", {name: (eng, (lambda e=eng: e.halpern_iterate(rate_iters))) for name, eng in engines.items()})
print(f"RESULT rate n={n} k={k} {prec} Halpern: native / split time per iteration = {med['native'] / med['split']:.4f}", flush=True)

# the RANGED functors where they are not needed: all-infinite q_upper against none, on the native engine
all_inf = torch.full((m,), float("inf"), dtype=dt, device=dev)


def window_with(qu):
    # (the library call itself: PdlpEngine.set_row_upper validates the vector, which synchronises)
    tp._native.check(native.lib.pdlp_set_row_upper(native.h, None if qu is None else qu.data_ptr()), "pdlp_set_row_upper")
    native.iterate(rate_iters, False)


native.set_row_upper(all_inf)                               # (validated once)
native.set_iterate(zeros(native.nl), zeros(native.ml))
native.set_step(0.9 / sig["native"], 1.0, 1.0, 0)
med = windows("cost", {"ranged": (native, lambda: window_with(all_inf)), "plain": (native, lambda: window_with(None))})
print(f"RESULT cost n={n} k={k} {prec}: RANGED functors at all-infinite q_upper / plain functors, time per iteration = "
      f"{med['ranged'] / med['plain']:.4f}", flush=True)

if os.environ.get("SOLVES", "1") != "0":
    limit, max_kkt = float(os.environ.get("TIME_LIMIT", "300")), int(os.environ.get("MAX_KKT", "400000"))
    native.set_row_upper(q_upper)
    for name, eng in engines.items():            # (two restart periods of each first: the adaptive and KKT kernels are loaded on first use)
        run_pdlp(eng, max_kkt=90, tol=tol, verbose=False, primal_update=True, adaptive=True, time_limit=limit, sigma=sig[name])
    for name, eng in engines.items():
        x, obj, it, nr, j, status, secs = run_pdlp(eng, max_kkt=max_kkt, tol=tol, verbose=False, primal_update=True, adaptive=True,
                                                   time_limit=limit, sigma=sig[name])
        print(f"RESULT solve n={n} k={k} tol={tol} {prec} form={name}: status={status} objective={obj:.6f} iterations={it} restarts={nr} "
              f"kkt_passes={j} seconds={secs:.3f} ms_per_iteration={1000 * secs / max(it, 1):.4f}", flush=True)
