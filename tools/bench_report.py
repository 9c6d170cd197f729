"""Cost of the solution report: ``PdlpEngine.report(CUR)`` against ``kkt(CUR)`` with fresh products (both multiply K'y and K x)
and against the ``pdlp_spmv`` pair, on one engine in one run; synchronised, best of ``--reps``.  Then one solve to ``--tol``
and the report's share of it.  Prints one JSON line.

    python tools/bench_report.py --n 1000000 --nnz_per_row 5
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchpdlp_amd as tp                        # noqa: E402
from torchpdlp_amd import _native as N            # noqa: E402
from torchpdlp_amd.solver import run_pdlp         # noqa: E402


def best(fn, eng, reps):
    fn()                                          # warm-up
    out = []
    for _ in range(reps):
        eng.synchronize()
        t0 = time.perf_counter()
        fn()
        eng.synchronize()
        out.append(time.perf_counter() - t0)
    return min(out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--nnz_per_row", type=int, default=5)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--tol", type=float, default=1e-4)
    p.add_argument("--no_solve", action="store_true")
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    lp = tp.gen_lp(a.n, a.n, a.nnz_per_row, seed=0, device=dev)
    K = tp.CsrPair(lp.m, lp.n, lp.rowptr, lp.colidx, lp.val)
    eng = tp.PdlpEngine.from_full(K, lp.c, lp.q, lp.l, lp.u, lp.m_ineq)
    eng.set_option(N.OPT_RUNNING_KKT, 0)          # every KKT pass multiplies both products
    eng.set_iterate(torch.zeros(lp.n, device=dev), torch.zeros(lp.m, device=dev))
    eng.set_step(0.01, 1.0, 1.0, 0)
    eng.iterate(5, False)
    x, y = eng.buffer(N.BUF_X_CUR), eng.buffer(N.BUF_Y_CUR)
    t_kkt = best(lambda: eng.kkt(N.CUR, 1.0), eng, a.reps)
    t_rep = best(lambda: eng.report(N.CUR), eng, a.reps)
    t_spmv = best(lambda: (eng.spmv(x, False), eng.spmv(y, True)), eng, a.reps)
    es, nnz = eng.dtype.itemsize, int(lp.val.numel())
    kkt_bytes = 2 * nnz * (es + 4) + (lp.n + lp.m) * 8 * 2 + (6 * lp.n + 4 * lp.m) * es          # items twice, row pointers, vectors
    extra = 3 * (lp.n + lp.m) * es                # two writes and one read of n + m values
    out = dict(n=lp.n, m=lp.m, nnz=nnz, kernels=eng.kernels, kkt_ms=t_kkt * 1e3, report_ms=t_rep * 1e3, spmv_pair_ms=t_spmv * 1e3,
               ratio_report_kkt=t_rep / t_kkt, ratio_report_spmv_pair=t_rep / t_spmv, byte_ratio=(kkt_bytes + extra) / kkt_bytes)
    if not a.no_solve:
        eng.set_option(N.OPT_RUNNING_KKT, 1)
        t0 = time.perf_counter()
        res = run_pdlp(eng, tol=a.tol, verbose=False, primal_update=True, adaptive=True, seed=0)
        eng.synchronize()
        total = time.perf_counter() - t0
        t_end = best(lambda: eng.report(N.CUR), eng, a.reps)
        out.update(solve_s=total, solve_status=res[5], solve_iterations=res[2], report_share_of_solve=t_end / (total + t_end))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
