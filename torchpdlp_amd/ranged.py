"""Two-sided constraint rows, ``q <= K x <= q_upper`` on the inequality rows: what the host does about them -- the validation of
``q_upper`` (before any device work), the vector whose 2-norm replaces ``||q||`` in the start value of the primal weight and in the
termination test, and the split twin of a two-sided LP (each two-sided row entered twice, as the MPS reader does), which tools and
tests compare the native form against.  The arithmetic itself is in the library (include/pdlp_hip.h, pdlp_set_row_upper)."""
from __future__ import annotations

import torch

from .compose import RANGED_REFUSED as REFUSED     # noqa: F401  (the text of the refusals, under its name here)


def check_row_upper(q, q_upper, m_ineq: int):
    """``q_upper`` as a 1-D tensor like ``q`` (same device and dtype), or None.  Inequality rows (``i < m_ineq``): ``q_i`` finite and
    ``q_upper_i >= q_i`` (``+inf``: a one-sided row, ``== q_i``: behaves as an equality row); equality rows: ``+inf`` or ``q_i`` (not
    read by the solver).  ``ValueError`` for a wrong length, ``q_upper_i < q_i``, NaN and ``-inf``."""
    if q_upper is None:
        return None
    q = torch.as_tensor(q).reshape(-1)
    qu = torch.as_tensor(q_upper).to(device=q.device, dtype=q.dtype).reshape(-1)
    if qu.numel() != q.numel():
        raise ValueError(f"q_upper has {qu.numel()} entries for {q.numel()} rows")
    m_ineq = int(m_ineq)
    if bool(torch.isnan(qu).any()) or bool((qu == -torch.inf).any()):
        raise ValueError("q_upper holds NaN or -inf (a row without an upper side has +inf)")
    lo, hi = q[:m_ineq], qu[:m_ineq]
    if not bool(torch.isfinite(lo).all()):
        raise ValueError("q must be finite on the inequality rows (a row without a lower side is entered negated)")
    if bool((hi < lo).any()):
        raise ValueError("q_upper < q on an inequality row")
    eq, eu = q[m_ineq:], qu[m_ineq:]
    if not bool(((eu == torch.inf) | (eu == eq)).all()):
        raise ValueError("q_upper on an equality row must be +inf or equal to q")
    return qu


def norm_vector(q, q_upper, m_ineq: int):
    """the vector whose 2-norm stands for ``||q||``: ``q_i`` where ``q_upper_i`` is ``+inf`` or the row is an equality row,
    ``max(|q_i|, |q_upper_i|)`` on two-sided rows; ``q`` itself without ``q_upper``"""
    if q_upper is None:
        return q
    q, qu = q.reshape(-1), q_upper.reshape(-1)
    two = torch.isfinite(qu)
    two[int(m_ineq):] = False
    return torch.where(two, torch.maximum(q.abs(), qu.abs()), q)


def split_rows(A, q, q_upper, m_ineq: int):
    """The split twin of a two-sided LP, host side (``A``: scipy sparse, ``q`` / ``q_upper``: numpy): every inequality row with a
    finite ``q_upper`` is followed by its negation with right-hand side ``-q_upper``.  -> ``(A_split, q_split, m_ineq_split, first)``
    with ``first[i]`` the split row that is row ``i``; a negated copy sits at ``first[i] + 1``."""
    import numpy as np
    import scipy.sparse as sp
    A = sp.csr_matrix(A)
    m = A.shape[0]
    two = np.isfinite(q_upper)
    two[int(m_ineq):] = False
    reps = 1 + two.astype(np.int64)
    first = np.concatenate(([0], np.cumsum(reps)[:-1]))
    src = np.repeat(np.arange(m), reps)
    sign = np.ones(src.size)
    sign[first[two] + 1] = -1.0
    qs = np.asarray(q, np.float64)[src].copy()
    qs[first[two] + 1] = -np.asarray(q_upper, np.float64)[two]
    As = (sp.diags(sign) @ A[src]).tocsr()
    As.sort_indices()
    return As, qs, int(m_ineq) + int(two.sum()), first
