"""The switches ``halpern``, ``q_upper``, ``quad_diag`` and ``quad_matrix`` against the forms they do not have: the refusals' text and the rule (the library: PDLP_ERR_STATE)."""
HALPERN_REFUSED = ("halpern=True runs the fixed step on one GPU in float32 or float64: not with adaptive, adaptive_retry, "
                   "infeasibility_detect, mixed precision or a communicator")
RANGED_REFUSED = ("q_upper (two-sided rows) runs on one GPU in float32 or float64: not with mixed precision, a communicator, "
                  "infeasibility_detect, fishnet or adaptive_retry")
QUAD_REFUSED = ("quad_diag (diagonal quadratic objective) runs on one GPU in float32 or float64: not with mixed precision, a communicator, "
                "direct_exchange, infeasibility_detect, fishnet or adaptive_retry")
QMAT_REFUSED = ("quad_matrix (sparse quadratic objective) runs the fixed, linearised step on one GPU in float32 or float64: not with "
                "adaptive, halpern, adaptive_retry, infeasibility_detect, mixed precision, a communicator, direct_exchange or fishnet")
QUAD_STEPS = ("fixed", "adaptive")


def check_quad_step(quad_step, quad_matrix) -> str:
    """``quad_step`` as given to a solve: one of ``QUAD_STEPS``, and "adaptive" (the step-size rule with the measured curvature
    ``dx'Q dx``, pdlp_objective_iterate) only with ``quad_matrix`` (``ValueError`` otherwise: the callers check before any device
    work).  What ``quad_matrix`` itself refuses stays refused under either value (``check_composition``)."""
    if quad_step not in QUAD_STEPS:
        raise ValueError(f"unknown quad_step {quad_step!r}: one of {', '.join(map(repr, QUAD_STEPS))}")
    if quad_step != "fixed" and not quad_matrix:
        raise ValueError(f"quad_step={quad_step!r} is a step rule of the sparse quadratic objective: it needs quad_matrix")
    return quad_step


def check_composition(*, halpern=False, q_upper=False, quad_diag=False, quad_matrix=False, adaptive=False, adaptive_retry=False,
                      infeasibility_detect=False, mixed=False, comm=False, fishnet=False, direct_exchange=False):
    """``ValueError`` with the switch's message if a switch that is on meets a form it does not have (arguments by truth value; an
    entry point leaves out what it has no flag for).  More than one refusal: Halpern, then ``q_upper``, then ``quad_diag``, then
    ``quad_matrix``."""
    one_gpu_only = adaptive_retry or infeasibility_detect or mixed or comm or direct_exchange
    if halpern and (adaptive or one_gpu_only):         # (only the fixed step; it does run behind a fishnet start)
        raise ValueError(HALPERN_REFUSED)
    if q_upper and (one_gpu_only or fishnet):
        raise ValueError(RANGED_REFUSED)
    if quad_diag and (one_gpu_only or fishnet):
        raise ValueError(QUAD_REFUSED)
    if quad_matrix and (adaptive or halpern or one_gpu_only or fishnet):      # (the linearised step: fixed, and not reflected)
        raise ValueError(QMAT_REFUSED)
