"""``solve_lp``: one call from an MPS file (or arrays) to a solution, the flow of the reference's driver
(``/root/reference/PDLP/main.py:85-137``) and of its older ``pdlp_solver`` wrapper
(``/root/reference/Packages/PDLP_without_presolve_infeasibility.py:748-789``) on the MI355X path."""
from __future__ import annotations

import os
import time as _time
from dataclasses import dataclass
from typing import Optional, Union

import torch

from .compose import check_quad_step
from .mps import mps_to_ranged_form, mps_to_standard_form
from .precondition import Scaling, equilibrate_matrix, ruiz_precondition, ruiz_precondition_batch
from .solver import check_composition, check_quad_diag, check_quad_matrix, check_row_upper, is_mixed, pdlp_algorithm, resolve_device
from .sparse import CsrPair


@dataclass
class LPResult:
    x: torch.Tensor            # (n, 1) primal solution of the ORIGINAL problem (un-scaled when preconditioned)
    objective: float           # c'x of the original problem (+ 1/2 x'Dx, + 1/2 x'Qx with quad_diag / quad_matrix)
    iterations: int            # k
    restarts: int              # n
    kkt_passes: int            # j
    status: str                # "Solved" | "Unsolved (KKT passes limit exceeded)" | "Unsolved (Time limit exceeded)"
                               # | "DUAL_INFEASIBLE" | "PRIMAL_INFEASIBLE" (only with infeasibility_detect)
    time: float                # seconds, preconditioning included (main.py:107,136)
    # the solution report (solve_lp(report=True), the default), all of the ORIGINAL problem; None without it.  Conventions, for the
    # form K x >= q with y >= 0 on the inequality rows: y_i = d(objective)/d(q_i); reduced cost lam_j > 0: x_j at its lower bound,
    # lam_j < 0: at its upper bound
    y: Optional[torch.Tensor] = None                # (m, 1) dual values
    reduced_costs: Optional[torch.Tensor] = None    # (n, 1) lam = project_lambda_box(c - K'y) (helpers.py:3-39,75-79)
    row_activity: Optional[torch.Tensor] = None     # (m, 1) K x
    dual_objective: Optional[float] = None          # q'y + l'max(lam,0) + u'min(lam,0) over the finite bounds (helpers.py:93-95)
    primal_residual: Optional[float] = None         # ||[K_eq x - q_eq; min(K_in x - q_in, 0)]|| (helpers.py:87-91)
    dual_residual: Optional[float] = None           # ||c - K'y - lam|| (helpers.py:84)
    gap: Optional[float] = None                     # dual_objective - objective, signed as the reference's (helpers.py:94)
    # the left-hand sides of the solver's check_termination (helpers.py:110-128): compare with tol; "Solved" means all three pass.
    # ||q||, ||c|| are the norms that test is given (pdhg.py:19-20): of the original q and c, or -- like the reference -- of the
    # Ruiz-scaled ones when preconditioned (the residuals above are of the original problem either way)
    rel_primal_residual: Optional[float] = None     # primal_residual / (1 + ||q||)
    rel_dual_residual: Optional[float] = None       # dual_residual / (1 + ||c||)
    rel_gap: Optional[float] = None                 # gap / (1 + |objective| + |dual_objective|)

    def as_tuple(self):
        """the reference's result tuple (pdhg.py:181)"""
        return self.x, self.objective, self.iterations, self.restarts, self.kkt_passes, self.status, self.time


def report_fields(rep: Optional[dict]) -> dict:
    """the report fields of ``LPResult`` / ``BatchResult`` from a solver report (``pdlp_algorithm(report=...)``: scalars, or a
    batch's [B] arrays).  The relative figures divide by the norms the solver's termination test was given (``q_norm``, ``c_norm``
    of the report), so they ARE the left-hand sides of its check_termination call: "Solved" means all three pass ``tol``."""
    if not rep:
        return {}
    import numpy as np
    f = lambda v: float(v) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)
    pr, dr, gap, p, d = (f(rep[k]) for k in ("pr", "dr", "gap", "p", "d_adj"))
    return dict(y=rep["y"], reduced_costs=rep["reduced_costs"], row_activity=rep["row_activity"], dual_objective=d,
                primal_residual=pr, dual_residual=dr, gap=gap, rel_primal_residual=pr / (1 + f(rep["q_norm"])),
                rel_dual_residual=dr / (1 + f(rep["c_norm"])), rel_gap=gap / (1 + abs(p) + abs(d)))


def solve_lp(problem: Union[str, os.PathLike, tuple], device=None, tol: float = 1e-4, precondition: bool = False,
             primal_weight_update: bool = False, adaptive_stepsize: bool = False, max_kkt: int = 100_000,
             time_limit: float = 3600, verbose: bool = False, restart_period: int = 40, dtype=torch.float32,
             seed: Optional[int] = None, compat: bool = True, x_init=None, y_init=None, trace=None,
             fishnet: bool = False, comm=None, infeasibility_detect: bool = False, infeas_tol: float = 1e-4,
             precision: Optional[str] = None, adaptive_retry: bool = False, direct_exchange: bool = False,
             report: bool = True, pock_chambolle: bool = False, halpern: bool = False, q_upper=None,
             ranged_rows: bool = False, quad_diag=None, halpern_restart: str = "kkt", quad_matrix=None,
             quad_norm: Optional[float] = None, quad_step: str = "fixed") -> LPResult:
    """Solve ``min c'x, K[:m_ineq]x >= q[:m_ineq], K[m_ineq:]x = q[m_ineq:], l <= x <= u`` on the current HIP device.

    ``problem`` is an MPS path or ``(c, K, q, m_ineq, l, u)`` with ``K`` dense / COO / scipy-sparse / ``CsrPair``.
    Flags carry the reference CLI's names (main.py:11-39); ``adaptive_retry`` (not in the reference's CLI) is ``pdlp_algorithm``'s.  ``dtype=torch.float64`` is the mode for tolerances
    below float32 resolution (the reference is float32 only); ``precision="mixed"`` (the problem is then read in float64) is the
    fast way there: float32 matrix entries under float64 vectors, iterations on the float32 kernels (``pdlp_algorithm``).
    ``infeasibility_detect`` runs the reference's detector
    (enhancements.py:80-161) after every iteration, with its behaviour as it is.  Under ``torchrun`` (one process per GPU, process
    group initialised) pass ``comm=True``: every rank reads the same problem ON THE HOST, puts only its row blocks of K and K'
    on its GPU (the Ruiz sweeps run on the shards), and all return the full solution -- no GPU ever holds the whole LP.
    ``report`` (default on): the result also carries the dual values, reduced costs, row activities and the residuals and gap of
    the ORIGINAL problem at the returned point, whatever the status (two products at the end of the solve; ``LPResult``'s fields
    say the conventions); ``report=False`` leaves them ``None``.
    ``direct_exchange`` (sharded solves, the ranks of ONE node, at most 8): the iterations run without collectives -- every half-step
    stores its block straight into the other ranks' memory over HIP IPC / xGMI (``PdlpEngine.enable_peer_exchange``, DESIGN.md
    section 5); connected and cross-checked against the collective-driven loop first, which stays in charge if anything differs.
    ``pock_chambolle`` (only with ``precondition``; not in the reference): PDLP's second scaling step, one Pock-Chambolle pass with
    alpha = 1 after the Ruiz sweeps -- rows and columns divided by the square roots of their 1-norms
    (``precondition.pock_chambolle_pass``).  It composes into the same ``D_col``, ``D_row``, so the solution and
    the report are un-scaled as with Ruiz alone.  Sharded solves do not have it yet and raise ``ValueError``.
    ``halpern`` (not in the reference): the restarted, reflected Halpern iteration instead of averaged PDHG, with the fixed step
    (``pdlp_algorithm``).  Works with ``precondition``, ``pock_chambolle``, ``primal_weight_update``,
    ``x_init`` / ``y_init`` and ``fishnet``; ``ValueError`` with ``adaptive_stepsize``, ``adaptive_retry``, ``infeasibility_detect``,
    ``precision="mixed"`` and for sharded solves (``comm``).  ``halpern_restart="fixed_point"`` (default "kkt"; needs ``halpern``):
    its restart checks look at the fixed-point residual ``||z - T(z)||_P`` of the Halpern iterate, the criterion of the rHPDHG papers,
    instead of the candidate's KKT error -- one product per check and no KKT pass; ``ValueError`` (before any
    device work) for another value or without ``halpern``.
    ``q_upper`` (length m; not in the reference): two-sided rows, ``q_i <= (K x)_i <= q_upper_i`` on the inequality rows, each
    entered ONCE instead of as two ``>=`` rows.  ``+inf`` is an ordinary row, ``q_upper_i == q_i`` behaves as
    an equality row; on the equality rows the entry must be ``+inf`` or ``q_i`` and is ignored.  In the report ``y_i > 0`` says the
    lower side of a two-sided row is active, ``y_i < 0`` the upper side.  ``ranged_rows=True`` (MPS paths): the ``RANGES`` rows of
    the file are read that way (``mps_to_ranged_form``) instead of being split.  Both work with ``precondition``,
    ``pock_chambolle``, ``primal_weight_update``, ``adaptive_stepsize``, ``halpern``, ``x_init`` / ``y_init`` and ``report`` in
    float32 and float64; ``ValueError`` (before any device work) for a malformed ``q_upper`` and together with
    ``precision="mixed"``, ``comm``, ``infeasibility_detect``, ``fishnet`` and ``adaptive_retry``.
    ``quad_diag`` (length n, ``d >= 0``; not in the reference): a separable quadratic term in the objective,
    ``min c'x + 1/2 sum_j d_j x_j^2`` over the same constraints: ridge-regularised LPs, the proximal term
    ``rho/2 ||x - xbar||^2`` of an outer loop (``d = rho``, ``c - rho xbar``), diagonal-risk models.  ``objective`` is then the quadratic
    objective, ``dual_objective`` its dual ``q'y + l'lam+ + u'lam- - 1/2 x'Dx`` and ``reduced_costs`` are
    ``project_lambda_box(c + Dx - K'y)``.  Works with ``precondition``, ``pock_chambolle``, ``primal_weight_update``,
    ``adaptive_stepsize``, ``halpern``, ``q_upper`` / ``ranged_rows``, ``x_init`` / ``y_init`` and ``report`` in float32 and float64;
    ``ValueError`` (before any device work) for a malformed vector and together with ``precision="mixed"``, ``comm``,
    ``direct_exchange`` (a flag of sharded solves), ``infeasibility_detect``, ``fishnet`` and ``adaptive_retry``.  With an MPS path the
    vector's length can only be compared with ``n`` after the file is read, which puts the problem on the device; everything else
    about it is checked first.  MPS ``QUADOBJ`` / ``QMATRIX`` sections are not read.
    ``quad_matrix`` (n x n, anything ``CsrPair.from_any`` takes; not in the reference): a general convex quadratic objective,
    ``min c'x + 1/2 x'Qx`` with ``Q`` sparse, symmetric and positive semidefinite: a factor covariance, a
    least-squares term, MPC.  Symmetry, the size, finiteness and a non-negative diagonal are checked; POSITIVE SEMIDEFINITENESS IS THE
    CALLER'S DUTY.  The solver takes the linearised step with a fixed step size that follows the primal weight (``rules.qp_eta``);
    ``quad_norm`` overrides its estimate of ``||Q||_2`` (of the scaled ``Q`` when ``precondition``).  ``objective`` is
    ``c'x + 1/2 x'Qx`` (``+ 1/2 x'Dx`` with ``quad_diag`` too), ``dual_objective`` is ``q'y + l'lam+ + u'lam- - 1/2 x'Qx (- 1/2 x'Dx)``
    and ``reduced_costs`` are ``project_lambda_box(c + Qx + Dx - K'y)``; the returned ``x`` is projected onto ``[l, u]`` (it moves by
    the rounding of the averaged iterate, a few eps; the objective and the residuals are those of the point before).  Works with ``precondition``, ``pock_chambolle``,
    ``primal_weight_update``, ``q_upper`` / ``ranged_rows``, ``quad_diag``, ``x_init`` / ``y_init`` and ``report`` in float32 and
    float64, with ``K`` on any product form; ``ValueError`` (before any device work) for a malformed matrix and together with
    ``adaptive_stepsize``, ``halpern``, ``adaptive_retry``, ``infeasibility_detect``, ``precision="mixed"``, ``comm``,
    ``direct_exchange`` and ``fishnet``.  With an MPS path the size is compared with ``n`` once the file is read.
    ``quad_step`` ("fixed", the default, or "adaptive"; with ``quad_matrix``): "adaptive" runs the same linearised step under an
    adaptive step size -- the rule of ``adaptive_stepsize`` with the curvature ``dx'Q dx`` measured along every step in its
    denominator, so the step follows the directions actually taken instead of 0.9 of the worst case over ``||K||`` and ``||Q||``
    (DESIGN.md section 4.5.1); it starts from ``rules.qp_eta``, costs the fixed step's three products per iteration and composes
    with everything ``quad_matrix`` composes with.  ``ValueError`` (before any device work) for another value, without
    ``quad_matrix``, and together with what ``quad_matrix`` refuses -- ``adaptive_stepsize`` itself included.
    """
    _check_pock_chambolle(pock_chambolle, precondition)
    from .solver import check_halpern_restart
    check_halpern_restart(halpern_restart, halpern)
    check_quad_step(quad_step, quad_matrix is not None)
    from_file = isinstance(problem, (str, os.PathLike))
    if ranged_rows and (not from_file or q_upper is not None):
        raise ValueError("ranged_rows=True reads the RANGES rows of an MPS path; arrays carry q_upper themselves")
    if q_upper is not None or ranged_rows or quad_diag is not None or quad_matrix is not None:
        is_mixed(precision)                     # (an unknown precision is its own error)
    check_composition(halpern=halpern, q_upper=q_upper is not None or ranged_rows, quad_diag=quad_diag is not None,
                      quad_matrix=quad_matrix is not None, adaptive=adaptive_stepsize, adaptive_retry=adaptive_retry, infeasibility_detect=infeasibility_detect,
                      mixed=precision is not None, comm=comm not in (None, False), fishnet=fishnet, direct_exchange=direct_exchange)
    if q_upper is not None:
        check_row_upper(problem[2], q_upper, problem[3])
    # (an MPS path: shape, sign and finiteness now, the length once the file is read)
    quad_diag = check_quad_diag(quad_diag, None if from_file or quad_diag is None else torch.as_tensor(problem[0]).numel())
    quad_matrix = check_quad_matrix(quad_matrix, None if from_file or quad_matrix is None else torch.as_tensor(problem[0]).numel())
    device = resolve_device(device)
    if is_mixed(precision):
        dtype = torch.float64
    # what pdlp_algorithm and run_pdlp are both told, under their names for it
    run = dict(max_kkt=max_kkt, tol=tol, restart_period=restart_period, precondition=precondition, primal_update=primal_weight_update,
               adaptive=adaptive_stepsize, time_limit=time_limit, trace=trace, infeasibility_detect=infeasibility_detect,
               infeas_tol=infeas_tol, adaptive_retry=adaptive_retry)
    if halpern:
        run["halpern"] = True
    if halpern_restart != "kkt":
        run["halpern_restart"] = halpern_restart
    if comm is not None and not fishnet:
        from .engine import Comm
        cm = Comm() if comm is True else comm
        if cm.world > 1:
            if pock_chambolle:
                raise ValueError("pock_chambolle has no sharded form yet (the pass needs the sweeps' gather of the full factor "
                                 "vectors): solve on one GPU, or with precondition alone")
            return _solve_lp_sharded(problem, cm, device, run, dtype=dtype, verbose=verbose, seed=seed, compat=compat, x_init=x_init,
                                     y_init=y_init, precision=precision, direct_exchange=direct_exchange, report=report)
    if ranged_rows:
        c, K, q, m_ineq, l, u, q_upper = mps_to_ranged_form(os.fspath(problem), device=device, verbose=verbose, compat=compat, dtype=dtype)
    else:
        c, K, q, m_ineq, l, u = load_problem(problem, device, dtype, verbose, compat)
    time_used, data_precond = 0.0, None
    if quad_diag is not None:
        quad_diag = check_quad_diag(quad_diag, c.numel())                # (a problem read from a file: its n is known only now)
    if quad_matrix is not None:
        quad_matrix = check_quad_matrix(quad_matrix, c.numel()).to(device=device, dtype=dtype)
    Ks, cs, qs, ls, us, qus, ds, Qs = K, c, q, l, u, q_upper, quad_diag, quad_matrix
    if precondition and (quad_diag is not None or quad_matrix is not None):
        Ks, cs, qs, ls, us, *more, data_precond, time_used = ruiz_precondition(c, K, q, l, u, device=device, pock_chambolle=pock_chambolle,
                                                                               q_upper=q_upper, quad_diag=quad_diag, quad_matrix=quad_matrix)
        # (the optional values follow u_s in this order, each only when it was given)
        qus, ds, Qs = (more.pop(0) if v is not None else None for v in (q_upper, quad_diag, quad_matrix))
    elif precondition and q_upper is not None:
        Ks, cs, qs, ls, us, qus, data_precond, time_used = ruiz_precondition(c, K, q, l, u, device=device, pock_chambolle=pock_chambolle,
                                                                             q_upper=q_upper)
    elif precondition:                                                  # main.py:106-110
        Ks, cs, qs, ls, us, data_precond, time_used = ruiz_precondition(c, K, q, l, u, device=device, pock_chambolle=pock_chambolle)
    if fishnet:                                                         # main.py:114-125 (k=32 points rounds, 2^5 points)
        from .spectral_casting import spectral_cast
        t0 = _time.time()
        gen = None if seed is None else torch.Generator().manual_seed(int(seed))
        x_init, y_init = spectral_cast(Ks, cs, qs, ls, us, m_ineq, k=32, device=device, generator=gen)
        time_used += _time.time() - t0
    rep = {} if report else None
    x, obj, k, n, j, status, total = pdlp_algorithm(
        Ks, m_ineq, cs, qs, ls, us, device, verbose=verbose, data_precond=data_precond, time_used=time_used, x_init=x_init,
        y_init=y_init, seed=seed, comm=comm, precision=precision, report=rep, **({} if qus is None else dict(q_upper=qus)),
        **({} if ds is None else dict(quad_diag=ds)), **({} if Qs is None else dict(quad_matrix=Qs, quad_norm=quad_norm, quad_step=quad_step)), **run)
    if precondition:        # the reference returns the scaled iterate (quirk Q4); solve_lp un-scales: x = D_col x_s (pdhg.py:161)
        x = Scaling(*data_precond[:2]).unscale_x(x)
    if quad_matrix is not None:
        # The returned point is usually an averaged iterate, x_sum / eta_sum.  Of iterates that all sit on a bound this is the bound
        # only up to the rounding of the two running sums (about one eps per four iterations of the period),
        # and D_col (l / D_col) adds its own.  In exact arithmetic the average is inside the box: project it onto the caller's bounds.
        x = torch.clamp(x.reshape(-1), min=torch.as_tensor(l).to(x).reshape(-1), max=torch.as_tensor(u).to(x).reshape(-1)).view_as(x)
    return LPResult(x, obj, k, n, j, status, total, **report_fields(rep))


def _check_pock_chambolle(pock_chambolle, precondition):
    """the Pock-Chambolle pass is a second step of the preconditioner: asked for without it, it is an error (before any device work)"""
    if pock_chambolle and not precondition:
        raise ValueError("pock_chambolle=True needs precondition=True (the pass runs after the Ruiz sweeps)")


def load_problem(problem, device, dtype, verbose=False, compat=True):
    """``(c, K, q, m_ineq, l, u)`` with ``K`` a ``CsrPair`` from an MPS path or from such a tuple with ``K`` dense / COO /
    scipy-sparse / ``CsrPair``.  ``device=None``: a file is read to the host, given arrays stay where the caller has them."""
    if isinstance(problem, (str, os.PathLike)):
        return mps_to_standard_form(os.fspath(problem), device="cpu" if device is None else device, verbose=verbose, compat=compat,
                                    dtype=dtype)
    c, K, q, m_ineq, l, u = problem
    return c, CsrPair.from_any(K, device=device, dtype=dtype), q, m_ineq, l, u


def _solve_lp_sharded(problem, comm, device, run, *, dtype, verbose, seed, compat, x_init, y_init, precision, direct_exchange,
                      report=True) -> LPResult:
    """``solve_lp`` over the ranks of ``comm``: the problem is read (or taken) on the host by every rank, cut into blocks balanced
    by non-zeros, and only this rank's blocks go to its GPU; Ruiz (enhancements.py:4-71) runs on the shards, the solve is
    ``run_pdlp`` (with the options ``run``) on the sharded engine (pdhg.py:7-181), and every rank returns the full un-scaled solution."""
    from .distributed import engine_from_shard, gather_report, gather_solution, shard_arrays, start_blocks
    from .solver import run_pdlp
    verbose = verbose and comm.rank == 0
    c, K, q, m_ineq, l, u = load_problem(problem, None, dtype, verbose, compat)
    n, m = K.n, K.m
    sh = shard_arrays(K, c, q, l, u, m_ineq, comm.rank, comm.world, vec_dtype=dtype, balance="nnz")
    one = lambda t: t.to(device) if isinstance(t, torch.Tensor) else t
    mv = lambda v: tuple(one(t) for t in v) if isinstance(v, tuple) else one(v)
    sh = {k: (v if k == "part" else mv(v)) for k, v in sh.items() if v is not None}
    del K
    eng = engine_from_shard(sh, comm, precision=precision, precondition=run["precondition"])
    time_used = float(getattr(eng, "ruiz_seconds", 0.0))
    if direct_exchange:            # (every rank asks; the ranks agree on every step, and on any failure all stay on the loop)
        on = eng.enable_peer_exchange()
        if verbose:
            print("direct exchange:", "on" if on else "declined", "--", "; ".join(eng.peer_log))
    x_init, y_init = start_blocks(eng, x_init, y_init, n, m)     # (of the scaled problem when preconditioned, like main.py:114-130)
    rep = {} if report else None
    x, obj, k, nr, j, status, total = run_pdlp(eng, verbose=verbose, time_used=time_used, x_init=x_init, y_init=y_init,
                                               seed=0 if seed is None else seed, report=rep, **run)
    if run["precondition"]:
        x = Scaling(eng.d_col, eng.d_row).unscale_x(x)
    if rep is not None:
        rep = gather_report(eng, rep, n, m)
    return LPResult(gather_solution(eng, x, n).view(-1, 1), obj, k, nr, j, status, total, **report_fields(rep))


@dataclass
class BatchResult:
    x: torch.Tensor            # (n, B) primal solutions of the ORIGINAL problems (un-scaled when preconditioned)
    y: torch.Tensor            # (m, B) dual solutions (un-scaled)
    objective: "np.ndarray"    # (B,) c'x per LP
    iterations: "np.ndarray"   # (B,) k
    restarts: "np.ndarray"     # (B,) n
    kkt_passes: "np.ndarray"   # (B,) j
    status: list               # B status strings of the reference
    time: float                # seconds for the whole batch
    # the solution report per LP (solve_lp_batch(report=True), the default; LPResult's fields of the same names): (n, B) / (m, B)
    # tensors and (B,) arrays, of the ORIGINAL problems; None without it
    reduced_costs: Optional[torch.Tensor] = None
    row_activity: Optional[torch.Tensor] = None
    dual_objective: Optional["np.ndarray"] = None
    primal_residual: Optional["np.ndarray"] = None
    dual_residual: Optional["np.ndarray"] = None
    gap: Optional["np.ndarray"] = None
    rel_primal_residual: Optional["np.ndarray"] = None
    rel_dual_residual: Optional["np.ndarray"] = None
    rel_gap: Optional["np.ndarray"] = None

    def __len__(self):
        return len(self.status)

    def __getitem__(self, i) -> LPResult:
        r = LPResult(self.x[:, i:i + 1], float(self.objective[i]), int(self.iterations[i]), int(self.restarts[i]),
                     int(self.kkt_passes[i]), self.status[i], self.time)
        if self.reduced_costs is not None:
            r.y, r.reduced_costs, r.row_activity = self.y[:, i:i + 1], self.reduced_costs[:, i:i + 1], self.row_activity[:, i:i + 1]
            for name in ("dual_objective", "primal_residual", "dual_residual", "gap", "rel_primal_residual", "rel_dual_residual",
                         "rel_gap"):
                setattr(r, name, float(getattr(self, name)[i]))
        return r


_BATCH_UNSUPPORTED = ("comm", "fishnet", "infeasibility_detect", "adaptive_retry", "direct_exchange")


def solve_lp_batch(problem: Union[str, os.PathLike, tuple], c=None, q=None, l=None, u=None, *, device=None, tol: float = 1e-4,
                   precondition: bool = False, primal_weight_update: bool = False, adaptive_stepsize: bool = False,
                   max_kkt: int = 100_000, time_limit: float = 3600, restart_period: int = 40, dtype=torch.float32,
                   seed: Optional[int] = None, compat: bool = True, x_init=None, y_init=None, trace=None, verbose: bool = False,
                   group_width: Optional[int] = None, b0=None, report: bool = True, K_values=None, setup_times: Optional[dict] = None,
                   slots: Optional[int] = None, schedule: Optional[dict] = None, pock_chambolle: bool = False,
                   halpern: bool = False, **unsupported) -> BatchResult:
    """Solve B LPs that share ``K`` (and ``m_ineq``) of ``problem`` and differ in ``c``, ``q``, ``l``, ``u`` in one batch.

    ``K_values`` ``(nnz, B)``: a constraint matrix per LP.  The LPs then share only the sparsity pattern of ``problem``'s K (its row
    pointers and column indices, m, n, m_ineq); column b holds the non-zero values of LP b in the order of the problem's CSR values
    (``CsrPair.val``), a stored zero where LP b lacks the entry.  ``sparse.stack_matrices`` builds ``(pattern, values)`` from a list
    of matrices whose patterns differ.  The step size and, with ``precondition``, the Ruiz equilibration are then per LP
    (``setup_times`` receives ``ruiz_seconds`` and ``power_iteration_seconds``).  Device memory: ``2 * nnz * Bp * itemsize`` on top
    of the shared copy.

    ``slots`` < B streams the family through ``slots`` columns (a positive multiple of the group width): the LPs wait in index order,
    and after every restart check the columns whose LP has finished are handed to the next ones.  The results are those of the plain
    batch at the same ``group_width``, bit for bit, in input order; device memory is that of ``slots`` LPs (with ``K_values``:
    ``2 * nnz * slots * itemsize``) plus the results, and the 2-D arguments (``K_values`` included) may stay on the host: they are
    copied ``slots`` columns at a time.  ``time_limit`` is for the whole run: LPs still waiting when it expires come back with the
    time-limit status, ``iterations == 0`` and their start point.  ``K_values`` with ``precondition`` has no streamed form.
    ``schedule``: a dict that receives ``column``, ``admitted_at``, ``retired_at`` per LP.

    ``problem`` (an MPS path or ``(c, K, q, m_ineq, l, u)``) supplies K and the default vectors; each of ``c, q, l, u`` may be
    omitted, 1-D (shared) or 2-D ``(len, B)`` (one column per LP; the 2-D arguments must agree on B).  Every LP runs through the
    reference's ``pdlp_algorithm`` with the same flags, its own step sizes, primal weight, restarts and KKT-pass count; ``max_kkt``
    applies per LP, ``time_limit`` to the whole batch.  With ``precondition`` one Ruiz equilibration of K serves every LP and each
    column of c, q, l, u is scaled; ``pock_chambolle`` (only with ``precondition``) adds ``solve_lp``'s Pock-Chambolle pass to it, once for
    a shared K and per LP with ``K_values``.  ``report`` (default on): the reduced costs, row activities, residuals and gaps of every LP
    (``BatchResult``'s fields; ``res[i]`` passes them on).  ``trace``: a list that receives B dicts (``kkt``, ``omega``, ``restarts``).  Flags of
    ``solve_lp`` that have no batched form (sharding, fishnet, infeasibility detection, ``adaptive_retry``, the direct exchange,
    ``precision="mixed"``) raise ``ValueError``.

    ``halpern`` (not in the reference): the restarted, reflected Halpern iteration per LP instead of averaged PDHG, with the fixed
    step (``solve_lp``'s flag; ``BatchDriver``): one KKT pass per restart check instead of three.  Works with
    ``precondition``, ``pock_chambolle``, ``primal_weight_update``, ``x_init`` / ``y_init``, ``K_values``, ``slots``, ``report`` and
    ``trace`` in float32 and float64; ``ValueError`` with ``adaptive_stepsize``."""
    import numpy as np
    from .batch import HALPERN_BATCH_REFUSED, batch_size, check_slots, pdlp_algorithm_batch
    _check_pock_chambolle(pock_chambolle, precondition)
    if halpern and adaptive_stepsize:
        raise ValueError(HALPERN_BATCH_REFUSED)
    for name, v in unsupported.items():
        if name == "precision":
            if v is not None:
                raise ValueError(f"precision={v!r} has no batched form (float32 or float64 through dtype)")
        elif name == "quad_matrix":
            if v is not None:
                raise ValueError("quad_matrix has no batched form")
        elif name in _BATCH_UNSUPPORTED:
            if v:
                raise ValueError(f"{name} has no batched form")
        else:
            raise TypeError(f"solve_lp_batch() got an unexpected keyword argument {name!r}")
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"unsupported dtype {dtype}")
    if group_width is not None and group_width not in (8, 16, 32):
        raise ValueError("group_width must be 8, 16 or 32")

    def check_lengths(n0, m0):
        for name, v, ln in (("c", c, n0), ("q", q, m0), ("l", l, n0), ("u", u, n0), ("x_init", x_init, n0), ("y_init", y_init, m0)):
            _check_batch_arg(name, v, ln)

    from_file = isinstance(problem, (str, os.PathLike))
    if not from_file:                        # given arrays say their lengths before any device work, a file once it is read
        check_lengths(len(problem[0]), len(problem[2]))
    if K_values is not None:
        K_values = torch.as_tensor(K_values)
        _check_matrix_values(K_values, problem[1].nnz if not from_file and isinstance(problem[1], CsrPair) else None)
    B_given = batch_size(*(torch.as_tensor(v) for v in (c, q, l, u, K_values) if v is not None))
    _check_start_width(B_given, x_init, y_init)
    streamed = check_slots(slots, B_given, group_width, dtype, K_values is not None, precondition)
    device = resolve_device(device)
    c0, K, q0, m_ineq, l0, u0 = load_problem(problem, device, dtype, verbose, compat)
    if from_file:
        check_lengths(K.n, K.m)
    _check_matrix_values(K_values, K.nnz)    # (a file or a dense / COO matrix says its pattern once it is CSR)
    # (a streamed family's 2-D arguments stay where they are: they are staged per admission)
    stays = lambda v: streamed and v is not None and len(v.shape) == 2
    vec = lambda v, d: (torch.as_tensor(v).to(dtype) if stays(v) else
                        (torch.as_tensor(d).reshape(-1) if v is None else torch.as_tensor(v)).to(device=device, dtype=dtype))
    C_, Q, L, U = vec(c, c0), vec(q, q0), vec(l, l0), vec(u, u0)
    B = batch_size(C_, Q, L, U, K_values)
    time_used, data_precond, Ks, KsV, KsTV = 0.0, None, K, None, None
    if K_values is not None:
        KsV = K_values.to(dtype) if streamed else K_values.to(device=device, dtype=dtype)
    if precondition:                         # main.py:106-110: K equilibrated once, or each LP's matrix on its own; every column scaled
        if K_values is not None:
            KsV, KsTV, D_col, D_row, secs = ruiz_precondition_batch(K, KsV, device=device, pock_chambolle=pock_chambolle)
            scaling = Scaling(D_col, D_row, seconds=secs)
            if setup_times is not None:
                setup_times["ruiz_seconds"] = secs
        else:
            Ks, scaling = equilibrate_matrix(K, device, pock_chambolle=pock_chambolle)
        t0 = _time.time()
        C_, Q, L, U = scaling.scale(C_, Q, L, U)
        time_used, data_precond = scaling.seconds + _time.time() - t0, (scaling.d_col, scaling.d_row)
    traces = None
    if trace is not None:
        traces = [dict(kkt=[], omega=[], restarts=[]) for _ in range(B)]
    rep = {} if report else None
    X, Y, obj, k, n, j, status, total = pdlp_algorithm_batch(
        Ks, m_ineq, C_, Q, L, U, device, max_kkt=max_kkt, tol=tol, verbose=verbose, restart_period=restart_period,
        precondition=precondition, primal_update=primal_weight_update, adaptive=adaptive_stepsize, data_precond=data_precond,
        time_limit=time_limit, time_used=time_used, x_init=x_init, y_init=y_init, seed=seed, traces=traces, group_width=group_width,
        b0=b0, report=rep, K_values=KsV, KT_values=KsTV, setup_times=setup_times, slots=slots if streamed else None, schedule=schedule,
        halpern=halpern)
    if trace is not None:
        trace.extend(traces)
    if precondition:                         # x = D_col x_s, y = D_row y_s (pdhg.py:161-162), per LP with a matrix each
        X, Y = scaling.unscale_x(X), scaling.unscale_y(Y)
    fields = report_fields(rep)
    fields.pop("y", None)                    # (the report's y is the same un-scaled Y)
    return BatchResult(X, Y, np.asarray(obj), np.asarray(k), np.asarray(n), np.asarray(j), status, total, **fields)


def _check_start_width(B, x_init, y_init):
    """a 2-D start must have one column per LP (B comes from c, q, l, u)"""
    for name, v in (("x_init", x_init), ("y_init", y_init)):
        if v is not None and len(v.shape) == 2 and v.shape[1] != B:
            raise ValueError(f"{name} has {v.shape[1]} columns for a batch of {B} LPs")


def _check_matrix_values(v, nnz):
    """``K_values``: 2-D, one row per stored entry of the pattern (``nnz``: None while the pattern is not known yet)"""
    if v is None:
        return
    shape = tuple(v.shape)
    if len(shape) != 2 or shape[1] < 1 or (nnz is not None and shape[0] != nnz):
        raise ValueError(f"K_values must have shape ({'nnz' if nnz is None else nnz}, B), got {shape}")


def _check_batch_arg(name, v, ln):
    if v is None:
        return
    shape = tuple(v.shape)
    if len(shape) not in (1, 2) or shape[0] != ln or (len(shape) == 2 and shape[1] < 1):
        raise ValueError(f"{name} must have shape ({ln},) or ({ln}, B), got {shape}")
