#!/usr/bin/env python3
"""Batched solves against the single-LP engine, in one process on one MI355X (torchpdlp_amd/batch.py, pdlp_batch_*).

Rates: LP-iterations per second of ``pdlp_batch_iterate`` for B in --batches, against ``PdlpEngine.iterate`` on the same LP in the
same run, fixed and adaptive step, on a launch-bound 50k x 50k LP and on BASELINE configs[1] (1M x 1M), both 5 non-zeros per row
(``gen_lp(..., recipe="box")``, the batch varies q per LP).  Every timed region is warmed up first and ends in a device
synchronise; the best of --reps repetitions is reported.  End to end: the wall time of ``solve_lp_batch`` on a 32-LP
``gen_lp_family`` to 1e-4 against 32 sequential ``solve_lp`` calls (50k shape).  ``--per-lp-values`` runs the same shapes once more
with a matrix per LP over the shared pattern (``K_values``: every value perturbed by 1 %) beside the shared-matrix rates of the
same run, and the end-to-end comparison on a ``matrix_noise`` family (set-up -- the per-LP power iteration, the value populations
-- included on both sides).  Prints one JSON document.

    python tools/bench_batch.py                         # everything
    python tools/bench_batch.py --shapes 1m --batches 8 --skip-e2e --reps 1   # the rocprofv3 --kernel-trace --stats run
    python tools/bench_batch.py --per-lp-values         # + a matrix per LP
    python tools/bench_batch.py --stream 32             # a family of 256 LPs: streamed, chunked loop, one plain batch
    python tools/bench_batch.py --halpern               # the Halpern iteration per LP against the fixed-step batched iteration

``--stream SLOTS`` solves one ``gen_lp_family`` of ``--family`` LPs (50k x 50k) three ways in one process -- streamed through SLOTS
columns (``solve_lp_batch(slots=SLOTS)``), as the loop of plain ``solve_lp_batch`` calls over chunks of SLOTS LPs that a user writes
without it, and as one plain batch -- each timed ``--reps`` times after a warm-up, all at the group width the chunks get.  It
prints the three lists of wall times, the distribution of the per-LP iteration counts, and whether the three agree bit for bit.
``--spread F``: that fraction of the LPs starts at its built-in optimum (solved at its first check), which spreads the counts.

``--halpern`` measures ``solve_lp_batch(halpern=True)`` (nothing else is run).  Rate: on ONE ``BatchEngine`` per B in --batches
(default 32,8; the 50k shape), HIP events around ``iterate(steps, adaptive=False)`` and ``halpern_iterate(steps)``, alternating,
--reps windows each after a warm-up of both -- ms per LP-iteration and their ratio, with the spread of the windows.  End to end:
the 32-LP family solved with the fixed step and with ``halpern=True`` (primal weight on both sides): seconds, and per LP the
iterations and KKT passes of the two methods and their ratios.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import torchpdlp_amd as tp
from torchpdlp_amd.batch import BatchEngine

SHAPES = {"50k": 50_000, "1m": 1_000_000}
MAX_B = {"50k": 128, "1m": 32}


def timed(fn, reps):
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def bytes_per_lp_iteration(n, m, nnz, B, W, es=4):
    """the cost model of one fixed-step iteration per LP ("Batched solves"): the two matrices are streamed once per
    group of W columns and shared by its LPs (8 bytes per item + 8 per row pointer); every item gathers es bytes per LP (in
    segments of W values); the epilogues stream the LP's columns (primal: read x, x_sum, write x, x_prev, xbar, x_sum; dual: read
    y, y_sum, q, write y, y_prev, y_sum)"""
    groups = -(-B // W)
    matrix = groups * 2 * (nnz * 8 + (n + m) * 8) / B
    gathers = 2 * nnz * es
    stream = n * 6 * es + m * 7 * es
    return dict(matrix=matrix, gathers=gathers, stream=stream, total=matrix + gathers + stream)


def bytes_per_lp_iteration_per_lp_values(n, m, nnz, B, W, es=4):
    """the same with a matrix per LP: the shared stream keeps its indices and row pointers (4 + 8 bytes) and every item reads
    es bytes of ITS LP's value beside the gather -- 2 nnz es more per LP-iteration, as much as the gathers"""
    groups = -(-B // W)
    matrix = groups * 2 * (nnz * 4 + (n + m) * 8) / B
    values = 2 * nnz * es
    gathers = 2 * nnz * es
    stream = n * 6 * es + m * 7 * es
    return dict(matrix=matrix, values=values, gathers=gathers, stream=stream, total=matrix + values + gathers + stream)


def rates(shape, batches, steps, reps, warm, per_lp=False):
    rows = SHAPES[shape]
    dev = torch.device("cuda", 0)
    lp = tp.gen_lp(rows, rows, 5, seed=0, device=dev)
    K = tp.CsrPair(lp.m, lp.n, lp.rowptr, lp.colidx, lp.val)
    out = dict(shape=f"{rows}x{rows}", nnz=int(K.nnz), steps=steps, reps=reps)
    eng = tp.PdlpEngine.from_full(K, lp.c, lp.q, lp.l, lp.u, lp.m_ineq)
    sigma = tp.solver.estimate_sigma(eng, power_iters=20, seed=0)
    eta = 0.9 / sigma
    single = {}
    for adaptive in (False, True):
        eng.set_iterate(torch.zeros(lp.n, device=dev), torch.zeros(lp.m, device=dev))
        eng.set_step(eta, 1.0, 1.0, 0)
        eng.iterate(warm, adaptive)
        single["adaptive" if adaptive else "fixed"] = steps / timed(lambda: eng.iterate(steps, adaptive), reps)
    out["single_it_per_s"] = single
    del eng
    out["batch"] = []
    g = torch.Generator(device=dev).manual_seed(1)
    for B in batches:
        if B > MAX_B[shape]:
            continue
        Q = lp.q.view(-1, 1) * (1 + 0.01 * torch.randn(lp.m, B, generator=g, device=dev))
        be = BatchEngine(K, lp.m_ineq, lp.c, Q, lp.l, lp.u, B)
        row = dict(B=B, W=be.W, Bp=be.Bp)

        def measure(be, prefix):
            for adaptive in (False, True):
                be.start(np.full(B, eta, np.float32), np.ones(B, np.float32))
                be.iterate(warm, adaptive, 0)
                k0 = [warm]

                def go():
                    be.iterate(steps, adaptive, k0[0])
                    k0[0] += steps
                dt = timed(go, reps)
                key = "adaptive" if adaptive else "fixed"
                row[f"{prefix}{key}_lp_it_per_s"] = B * steps / dt
                row[f"{prefix}{key}_speedup"] = B * steps / dt / single[key]
                row[f"{prefix}{key}_us_per_iteration"] = dt / steps * 1e6

        measure(be, "")
        model = bytes_per_lp_iteration(lp.n, lp.m, int(K.nnz), B, be.W)
        row["model_bytes_per_lp_iteration"] = model
        row["fixed_model_GB_per_s"] = model["total"] * row["fixed_lp_it_per_s"] / 1e9
        if per_lp:
            del be
            V = K.val.view(-1, 1) * (1 + 0.01 * torch.randn(K.nnz, B, generator=g, device=dev))
            be = BatchEngine(K, lp.m_ineq, lp.c, Q, lp.l, lp.u, B, K_values=V)
            del V
            measure(be, "per_lp_values_")
            pm = bytes_per_lp_iteration_per_lp_values(lp.n, lp.m, int(K.nnz), B, be.W)
            row["per_lp_values_model_bytes_per_lp_iteration"] = pm
            row["per_lp_values_fixed_model_GB_per_s"] = pm["total"] * row["per_lp_values_fixed_lp_it_per_s"] / 1e9
            row["per_lp_values_fixed_rate_ratio"] = row["per_lp_values_fixed_lp_it_per_s"] / row["fixed_lp_it_per_s"]
            row["per_lp_values_model_rate_ratio"] = model["total"] / pm["total"]
        out["batch"].append(row)
        print(json.dumps(dict(shape=shape, **row)), file=sys.stderr, flush=True)
        del be
    return out


def end_to_end(B=32, rows=50_000):
    dev = torch.device("cuda", 0)
    f = tp.gen_lp_family(rows, rows, 5, B, seed=0)
    K = tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val).to(dev)
    C, Q, L, U = (v.to(dev) for v in (f.C, f.Q, f.L, f.U))
    prob = (C[:, 0], K, Q[:, 0], f.m_ineq, L[:, 0], U[:, 0])
    tp.solve_lp_batch(prob, C[:, :2], Q[:, :2], L[:, :2], U[:, :2], device=dev, seed=0, max_kkt=200)        # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = tp.solve_lp_batch(prob, C, Q, L, U, device=dev, seed=0, time_limit=600)
    torch.cuda.synchronize()
    t_batch = time.perf_counter() - t0
    t0 = time.perf_counter()
    seq = [tp.solve_lp((C[:, b], K, Q[:, b], f.m_ineq, L[:, b], U[:, b]), device=dev, seed=0, time_limit=600) for b in range(B)]
    torch.cuda.synchronize()
    t_seq = time.perf_counter() - t0
    rel = lambda a, b: abs(a - b) / (1 + abs(b))
    return dict(B=B, shape=f"{rows}x{rows}", batch_seconds=t_batch, sequential_seconds=t_seq, speedup=t_seq / t_batch,
                batch_solved=sum(s == "Solved" for s in res.status), sequential_solved=sum(r.status == "Solved" for r in seq),
                batch_iterations_max=int(res.iterations.max()), sequential_iterations_sum=int(sum(r.iterations for r in seq)),
                max_rel_obj_diff_vs_sequential=max(rel(res.objective[b], seq[b].objective) for b in range(B)))


def end_to_end_per_lp_values(B=32, rows=50_000, noise=0.05):
    """a ``matrix_noise`` family: one ``solve_lp_batch(K_values=...)`` against B sequential ``solve_lp`` calls, each over its own
    matrix (the transposed copy of every LP's matrix is built inside the timed region on both sides)"""
    dev = torch.device("cuda", 0)
    f = tp.gen_lp_family(rows, rows, 5, B, seed=0, matrix_noise=noise)
    K = tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val).to(dev)
    C, Q, L, U, V = (v.to(dev) for v in (f.C, f.Q, f.L, f.U, f.vals))
    prob = (C[:, 0], K, Q[:, 0], f.m_ineq, L[:, 0], U[:, 0])
    tp.solve_lp_batch(prob, C[:, :2], Q[:, :2], L[:, :2], U[:, :2], device=dev, seed=0, max_kkt=200, K_values=V[:, :2])        # warm-up
    torch.cuda.synchronize()
    times = {}
    t0 = time.perf_counter()
    res = tp.solve_lp_batch(prob, C, Q, L, U, device=dev, seed=0, time_limit=600, K_values=V, setup_times=times)
    torch.cuda.synchronize()
    t_batch = time.perf_counter() - t0
    t0 = time.perf_counter()
    seq = []
    for b in range(B):
        Kb = tp.CsrPair(f.m, f.n, K.rowptr, K.colidx, V[:, b].contiguous())
        seq.append(tp.solve_lp((C[:, b], Kb, Q[:, b], f.m_ineq, L[:, b], U[:, b]), device=dev, seed=0, time_limit=600))
    torch.cuda.synchronize()
    t_seq = time.perf_counter() - t0
    t0 = time.perf_counter()
    tp.precondition.ruiz_precondition_batch(K, V)
    torch.cuda.synchronize()
    t_ruiz = time.perf_counter() - t0
    rel = lambda a, b: abs(a - b) / (1 + abs(b))
    return dict(B=B, shape=f"{rows}x{rows}", matrix_noise=noise, batch_seconds=t_batch, sequential_seconds=t_seq, speedup=t_seq / t_batch,
                batch_solved=sum(s == "Solved" for s in res.status), sequential_solved=sum(r.status == "Solved" for r in seq),
                batch_iterations_max=int(res.iterations.max()), sequential_iterations_sum=int(sum(r.iterations for r in seq)),
                max_rel_obj_diff_vs_sequential=max(rel(res.objective[b], seq[b].objective) for b in range(B)),
                max_rel_obj_diff_vs_optimum=max(rel(res.objective[b], f.opt_obj[b]) for b in range(B)),
                power_iteration_seconds=times.get("power_iteration_seconds"), ruiz_per_lp_seconds_not_in_the_solve=t_ruiz)


def stream_family(slots, family, spread, reps, rows=50_000, only_streamed=False):
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    f = tp.gen_lp_family(rows, rows, 5, family, seed=0)
    print(f"family of {family} generated in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    K = tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val).to(dev)
    C, Q, L, U = (v.to(dev) for v in (f.C, f.Q, f.L, f.U))
    X0, Y0 = torch.zeros(f.n, family, device=dev), torch.zeros(f.m, family, device=dev)
    if spread > 0:
        step = max(1, round(1 / spread))
        X0[:, ::step], Y0[:, ::step] = f.X_opt[:, ::step].float().to(dev), f.Y_opt[:, ::step].float().to(dev)
    prob = (C[:, 0], K, Q[:, 0], f.m_ineq, L[:, 0], U[:, 0])
    W = tp.batch.group_width(slots, torch.float32)
    kw = dict(device=dev, seed=0, time_limit=600, group_width=W)
    cols = lambda a, b: dict(c=C[:, a:b], q=Q[:, a:b], l=L[:, a:b], u=U[:, a:b], x_init=X0[:, a:b], y_init=Y0[:, a:b])
    tp.solve_lp_batch(prob, **cols(0, 2 * slots), slots=slots, max_kkt=200, **kw)          # warm-up (every kernel of the three ways)
    torch.cuda.synchronize()

    def streamed():
        return [tp.solve_lp_batch(prob, **cols(0, family), slots=slots, **kw)]

    def chunked():
        return [tp.solve_lp_batch(prob, **cols(a, min(a + slots, family)), **kw) for a in range(0, family, slots)]

    def plain():
        return [tp.solve_lp_batch(prob, **cols(0, family), **kw)]

    out = dict(slots=slots, family=family, W=W, shape=f"{rows}x{rows}", spread=spread, reps=reps)
    results = {}
    for name, fn in (("streamed", streamed), ("chunked", chunked), ("plain", plain)):
        if only_streamed and name != "streamed":
            continue
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        results[name] = res
        out[f"{name}_seconds"] = times
        out[f"{name}_best"] = min(times)
        print(json.dumps({name: times}), file=sys.stderr, flush=True)
    cat = lambda rs, key: np.concatenate([np.asarray(getattr(r, key)) for r in rs])
    its = cat(results["streamed"], "iterations")
    out["iterations"] = dict(min=int(its.min()), p25=int(np.percentile(its, 25)), median=int(np.median(its)),
                             p75=int(np.percentile(its, 75)), max=int(its.max()), sum=int(its.sum()))
    out["solved"] = int(sum(s == "Solved" for r in results["streamed"] for s in r.status))
    if not only_streamed:
        # the iterations a column spends waiting for the slowest LP of its chunk / of the whole batch
        per_chunk = [int(r.iterations.max()) * len(r) for r in results["chunked"]]
        out["column_iterations"] = dict(useful=int(its.sum()), chunked=int(sum(per_chunk)), plain=int(its.max()) * family)
        out["streamed_over_chunked"] = out["streamed_best"] / out["chunked_best"]
        out["chunked_spread"] = (max(out["chunked_seconds"]) - min(out["chunked_seconds"])) / min(out["chunked_seconds"])
        same = lambda a, b: bool(torch.equal(torch.cat([r.x for r in a], 1), torch.cat([r.x for r in b], 1)) and
                                 (cat(a, "iterations") == cat(b, "iterations")).all())
        out["streamed_equals_plain"] = same(results["streamed"], results["plain"])
        out["chunked_equals_plain"] = same(results["chunked"], results["plain"])
    return out


def halpern_rates(batches, steps, rounds, warm, rows=50_000):
    """ms per LP-iteration of the two batched iterations on one engine, alternating windows timed by HIP events on its stream"""
    dev = torch.device("cuda", 0)
    lp = tp.gen_lp(rows, rows, 5, seed=0, device=dev)
    K = tp.CsrPair(lp.m, lp.n, lp.rowptr, lp.colidx, lp.val)
    eng = tp.PdlpEngine.from_full(K, lp.c, lp.q, lp.l, lp.u, lp.m_ineq)
    eta = 0.9 / tp.solver.estimate_sigma(eng, power_iters=20, seed=0)
    del eng
    g = torch.Generator(device=dev).manual_seed(1)
    out = []
    for B in batches:
        Q = lp.q.view(-1, 1) * (1 + 0.01 * torch.randn(lp.m, B, generator=g, device=dev))
        be = BatchEngine(K, lp.m_ineq, lp.c, Q, lp.l, lp.u, B)
        be.start(np.full(B, eta, np.float32), np.ones(B, np.float32))
        count = [0]

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            be.synchronize()
            e0.record(be.stream)
            fn()
            e1.record(be.stream)
            e1.synchronize()
            count[0] += steps
            return e0.elapsed_time(e1) / steps / B

        pdhg = lambda: be.iterate(steps, False, count[0])
        halp = lambda: be.halpern_iterate(steps, np.full(B, count[0], np.int64))
        be.iterate(warm, False, 0), be.halpern_iterate(warm, np.zeros(B, np.int64))
        timed(pdhg), timed(halp)                                    # warm-up of both
        ms = {"fixed": [], "halpern": []}
        for _ in range(rounds):
            ms["fixed"].append(timed(pdhg))
            ms["halpern"].append(timed(halp))
        spread = {k: (max(v) - min(v)) / float(np.median(v)) for k, v in ms.items()}
        row = dict(B=B, W=be.W, shape=f"{rows}x{rows}", steps=steps, ms_per_lp_iteration=ms, window_spread=spread,
                   halpern_over_fixed=float(np.median(ms["halpern"]) / np.median(ms["fixed"])),
                   halpern_over_fixed_per_window=[h / f for h, f in zip(ms["halpern"], ms["fixed"])])
        out.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del be
    return out


def halpern_end_to_end(B=32, rows=50_000):
    """the tool's 32-LP family with the fixed step and with halpern=True, primal weight on both sides"""
    dev = torch.device("cuda", 0)
    f = tp.gen_lp_family(rows, rows, 5, B, seed=0)
    K = tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val).to(dev)
    C, Q, L, U = (v.to(dev) for v in (f.C, f.Q, f.L, f.U))
    prob = (C[:, 0], K, Q[:, 0], f.m_ineq, L[:, 0], U[:, 0])
    out = dict(B=B, shape=f"{rows}x{rows}", tol=1e-4)
    res = {}
    for name, kw in (("fixed", {}), ("halpern", dict(halpern=True))):
        tp.solve_lp_batch(prob, C[:, :2], Q[:, :2], L[:, :2], U[:, :2], device=dev, seed=0, max_kkt=200, primal_weight_update=True, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = res[name] = tp.solve_lp_batch(prob, C, Q, L, U, device=dev, seed=0, time_limit=600, primal_weight_update=True, **kw)
        torch.cuda.synchronize()
        rel = lambda a, b: abs(a - b) / (1 + abs(b))
        out[name] = dict(seconds=time.perf_counter() - t0, solved=sum(s == "Solved" for s in r.status),
                         iterations=r.iterations.tolist(), kkt_passes=r.kkt_passes.tolist(), restarts=r.restarts.tolist(),
                         max_rel_obj_diff_vs_optimum=max(rel(r.objective[b], f.opt_obj[b]) for b in range(B)))
    for key in ("iterations", "kkt_passes"):
        h, p = np.asarray(getattr(res["halpern"], key), float), np.asarray(getattr(res["fixed"], key), float)
        out[f"{key}_ratio"] = dict(of_sums=float(h.sum() / p.sum()), of_max=float(h.max() / p.max()), per_lp_min=float((h / p).min()),
                                   per_lp_median=float(np.median(h / p)), per_lp_max=float((h / p).max()))
    out["seconds_ratio"] = out["halpern"]["seconds"] / out["fixed"]["seconds"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="50k,1m")
    ap.add_argument("--batches", default="1,8,32,128")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warm", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--per-lp-values", action="store_true", help="the same shapes with a matrix per LP (K_values) as well")
    ap.add_argument("--stream", type=int, default=0, metavar="SLOTS", help="a long family streamed through SLOTS columns, against "
                    "the loop over chunks of SLOTS and one plain batch (nothing else is run)")
    ap.add_argument("--family", type=int, default=256, help="LPs of the --stream family")
    ap.add_argument("--spread", type=float, default=0.0, help="fraction of the --stream family that starts at its optimum")
    ap.add_argument("--stream-only", action="store_true", help="--stream: the streamed solve alone (the kernel-trace run)")
    ap.add_argument("--halpern", action="store_true", help="the Halpern iteration per LP against the fixed-step batched iteration: "
                    "the rate on one engine (alternating windows) and the 32-LP family end to end (nothing else is run)")
    a = ap.parse_args()
    if a.halpern:
        batches = [32, 8] if a.batches == ap.get_default("batches") else [int(b) for b in a.batches.split(",")]
        doc = dict(device=torch.cuda.get_device_name(0), dtype="float32", halpern_rates=halpern_rates(batches, a.steps, a.reps, a.warm))
        if not a.skip_e2e:
            doc["halpern_end_to_end"] = halpern_end_to_end()
        print(json.dumps(doc, indent=1))
        return
    if a.stream:
        print(json.dumps(dict(device=torch.cuda.get_device_name(0), dtype="float32",
                              stream=stream_family(a.stream, a.family, a.spread, a.reps, only_streamed=a.stream_only)), indent=1))
        return
    batches = [int(b) for b in a.batches.split(",")]
    doc = dict(device=torch.cuda.get_device_name(0), dtype="float32", rates={})
    for s in a.shapes.split(","):
        doc["rates"][s] = rates(s, batches, a.steps, a.reps, a.warm, a.per_lp_values)
    if not a.skip_e2e:
        doc["end_to_end"] = end_to_end()
        if a.per_lp_values:
            doc["end_to_end_per_lp_values"] = end_to_end_per_lp_values()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
