#!/usr/bin/env python3
"""The Pock-Chambolle pass (solve_lp's pock_chambolle=True) measured against Ruiz alone.

    python tools/bench_pock_chambolle.py setup [n] [nnz_per_row]     # the pass against ONE Ruiz sweep on the bench LP's matrix
    python tools/bench_pock_chambolle.py family [n] [tol]            # a badly scaled LP with a known optimum, solved both ways

setup: HIP events around ``precondition._sweeps(max_iter=1)`` and ``precondition.pock_chambolle_pass`` on fresh copies of the same
matrix, one warm-up and three repeats each, float32.  (A sweep ends with its early-exit test, one host read; the pass has none.)
family: ``gen_lp_family``'s n x n LP with rows and columns multiplied by 10^U(-2, 2) (the optimum stays known), float32, adaptive
step and primal weight, seed 0: iterations, seconds and the objective's error with ``precondition`` alone and with the pass."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torchpdlp_amd as tp
from torchpdlp_amd import _native as N
from torchpdlp_amd import precondition as pc
from torchpdlp_amd.engine import _DT

dev = torch.device("cuda", 0)
mode = sys.argv[1] if len(sys.argv) > 1 else "setup"


def timed(fn, Kp, repeats=3):
    """ms of fn on a fresh copy of Kp each time (the copy is made outside the events); the first call is the warm-up"""
    lib, code = N.load(), _DT[Kp.dtype]
    stream = torch.cuda.current_stream(dev)
    out = []
    for _ in range(repeats + 1):
        Ks = Kp.clone()
        D_row = torch.ones(Ks.m, dtype=Ks.dtype, device=dev)
        D_col = torch.ones(Ks.n, dtype=Ks.dtype, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        e0.record(stream)
        fn(lib, code, stream.cuda_stream, Ks.m, Ks.n, (Ks.rowptr, Ks.colidx, Ks.val), (Ks.t_rowptr, Ks.t_colidx, Ks.t_val), D_row, D_col)
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
        del Ks
    return out[1:]


if mode == "setup":
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    t0 = time.time()
    lp = tp.gen_lp(n, n, k, seed=0, device=dev)
    Kp = tp.CsrPair(lp.m, lp.n, lp.rowptr, lp.colidx, lp.val)
    torch.cuda.synchronize()
    print(f"{n} x {n}, {Kp.nnz} non-zeros, built in {time.time() - t0:.1f} s", flush=True)
    sweep = timed(lambda *a: pc._sweeps(*a, 1, 1e-6), Kp)
    print(f"one Ruiz sweep: {' '.join(f'{t:.3f}' for t in sweep)} ms", flush=True)
    pas = timed(pc.pock_chambolle_pass, Kp)
    print(f"the pass      : {' '.join(f'{t:.3f}' for t in pas)} ms", flush=True)
    print(f"RESULT n={n} k={k}: pass / sweep = {np.median(pas) / np.median(sweep):.3f} (medians {np.median(pas):.3f} / {np.median(sweep):.3f} ms)")
else:
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 50_000
    tol = float(sys.argv[3]) if len(sys.argv) > 3 else 1e-4
    f = tp.gen_lp_family(n, n, 5, 1, seed=5, dtype=torch.float64)
    rng = np.random.default_rng(17)
    R = torch.from_numpy(10.0 ** rng.uniform(-2, 2, f.m))
    S = torch.from_numpy(10.0 ** rng.uniform(-2, 2, f.n))
    rows = torch.repeat_interleave(torch.arange(f.m), torch.diff(f.rowptr))
    val = (f.val * R[rows] * S[f.colidx.long()]).float()
    K = tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, val).to(dev)
    d = lambda v: v.float().to(dev)
    prob = (d(f.C[:, 0] * S), K, d(f.Q[:, 0] * R), f.m_ineq, d(f.L[:, 0] / S), d(f.U[:, 0] / S))
    opt = f.opt_obj[0]
    for pock in (False, True, False, True):
        r = tp.solve_lp(prob, device=dev, tol=tol, precondition=True, pock_chambolle=pock, primal_weight_update=True, adaptive_stepsize=True,
                        seed=0, max_kkt=int(os.environ.get("MAX_KKT", "400000")), time_limit=float(os.environ.get("TIME_LIMIT", "120")))
        print(f"RESULT family n={n} tol={tol} pock_chambolle={pock}: status={r.status} iterations={r.iterations} restarts={r.restarts} "
              f"time={r.time:.3f}s objective error {abs(r.objective - opt) / (1 + abs(opt)):.2e} rel_primal {r.rel_primal_residual:.2e} "
              f"rel_dual {r.rel_dual_residual:.2e}", flush=True)
