"""Diagonal quadratic objective, ``min c'x + 1/2 sum_j d_j x_j^2`` with ``d >= 0``: what the host does about it -- the validation of
``quad_diag`` (before any device work) and the text of the refusals.  The arithmetic itself is in the library (include/pdlp_hip.h,
pdlp_set_objective_diag); the preconditioner's part is ``Scaling.scale(..., quad_diag=)``: ``d_s = d D_col^2``."""
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
