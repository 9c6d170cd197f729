"""Quadratic objectives: what the host does about them -- the validation of the operands (before any device work) and the text of
the refusals.  ``quad_diag``: ``min c'x + 1/2 sum_j d_j x_j^2`` with ``d >= 0`` (include/pdlp_hip.h, pdlp_set_objective_diag; the
preconditioner's part is ``Scaling.scale(..., quad_diag=)``: ``d_s = d D_col^2``).  ``quad_matrix``: ``min c'x + 1/2 x'Qx`` with ``Q``
sparse, symmetric and positive semidefinite (pdlp_set_objective_matrix; ``Scaling.scale(..., quad_matrix=)``: ``D_col Q D_col``; the
step rule is ``rules.qp_eta``).  The arithmetic itself is in the library."""
from __future__ import annotations

import torch

from .compose import QUAD_REFUSED as REFUSED     # noqa: F401  (the text of the refusals, under its name here)


def check_quad_diag(d, n=None):
    """``quad_diag`` as a 1-D tensor of length ``n`` (a column ``(n, 1)`` is flattened), or None.  Every entry finite and ``>= 0``
    (0: the variable has no quadratic term).  ``ValueError`` for another shape or length, a negative entry, NaN and ``inf``.
    ``n=None``: everything but the length (a problem still in its file: its ``n`` is known only once it is read)."""
    if d is None:
        return None
    d = torch.as_tensor(d)
    if d.dim() == 2 and d.shape[1] == 1:
        d = d.reshape(-1)
    if d.dim() != 1:
        raise ValueError(f"quad_diag must be a vector (the diagonal of the quadratic term), got shape {tuple(d.shape)}")
    if n is not None and d.numel() != int(n):
        raise ValueError(f"quad_diag has {d.numel()} entries for {int(n)} variables")
    if d.is_complex() or d.dtype == torch.bool:
        raise ValueError(f"quad_diag must hold real numbers, got {d.dtype}")
    if not bool(torch.isfinite(d.double()).all()):
        raise ValueError("quad_diag holds NaN or inf")
    if bool((d < 0).any()):
        raise ValueError("quad_diag holds a negative entry (the objective must stay convex: d >= 0)")
    return d


def check_quad_matrix(Q, n=None):
    """``quad_matrix`` as a ``CsrPair`` (any form ``CsrPair.from_any`` accepts: dense / COO / CSR tensor, scipy sparse, ``CsrPair``;
    left where the caller has it), or None.  It must be ``n x n``, every stored entry finite, symmetric -- the pair's CSR arrays and
    those of its transposed copy are equal, pattern and values (so a ``CsrPair`` handed in needs ascending column indices in every
    row, as every other form gets them) -- and its diagonal ``>= 0``.  ``ValueError`` otherwise, before any device work on the solve.
    POSITIVE SEMIDEFINITENESS IS THE CALLER'S DUTY: it cannot be read off the entries, the iteration does not converge without it and
    nothing here or in the library checks it.  ``n=None``: everything but the size."""
    if Q is None:
        return None
    from .sparse import CsrPair
    Qp = CsrPair.from_any(Q)
    if Qp.m != Qp.n:
        raise ValueError(f"quad_matrix must be square, got {Qp.m} x {Qp.n}")
    if n is not None and Qp.n != int(n):
        raise ValueError(f"quad_matrix is {Qp.m} x {Qp.n} for {int(n)} variables")
    if Qp.val.is_complex() or not Qp.val.is_floating_point():
        raise ValueError(f"quad_matrix must hold real floating-point numbers, got {Qp.val.dtype}")
    if not bool(torch.isfinite(Qp.val).all()):
        raise ValueError("quad_matrix holds NaN or inf")
    if not (torch.equal(Qp.rowptr, Qp.t_rowptr) and torch.equal(Qp.colidx, Qp.t_colidx)):
        raise ValueError("quad_matrix is not symmetric: the pattern of Q differs from the pattern of Q'")
    if not torch.equal(Qp.val, Qp.t_val):
        raise ValueError("quad_matrix is not symmetric: Q and Q' differ in a value")
    rows = torch.repeat_interleave(torch.arange(Qp.n, device=Qp.device), (Qp.rowptr[1:] - Qp.rowptr[:-1]))
    diag = Qp.val[rows == Qp.colidx.long()]
    if bool((diag < 0).any()):
        raise ValueError("quad_matrix has a negative diagonal entry (the objective must stay convex: Q positive semidefinite)")
    return Qp
