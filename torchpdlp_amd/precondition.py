"""Ruiz equilibration, and PDLP's Pock-Chambolle pass after it, on the two CSR copies of K, on the device.

``equilibrate`` is the one body (``_sweeps``, then ``pock_chambolle_pass`` when asked; the ``pdlp_csr_*`` / ``pdlp_vec_*`` entry points
of the C ABI) and ``Scaling`` what it returns: the factors, and the one place that scales vectors by them and un-scales iterates.
``ruiz_precondition`` is the drop-in for the reference's (``/root/reference/PDLP/enhancements.py:4-71``), which is dense-only
(``torch.linalg.norm(K, ord=inf, dim=...)`` does not take sparse input) and cannot run at the benchmark sizes.  Each sweep is: row
factors of K (sqrt of the row's max |.|, 1 when < eps), divide K's rows and K''s columns by them; the same from K' for the columns.
``pock_chambolle=True`` adds one pass by the square roots of the row and column 1-norms (``pock_chambolle_pass``; not in the reference).
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass

import torch

from . import _native as N
from .engine import _DT
from .sparse import CsrPair, as_vec, resolve_device


def _sweeps(lib, code, stream, rows_K, rows_KT, K_blk, KT_blk, D_row, D_col, max_iter, eps, comm=None, r0=0, c0=0):
    """The Ruiz sweeps (enhancements.py:45-62) on one rank's row block of K (``rows_K`` rows, global column indices) and of K'
    (``rows_KT`` rows, global row indices), in place.  Row norms of K and of K' are rank local; what the other matrix copy needs
    of them -- the factors of ALL constraints resp. ALL variables, for its columns -- is one all-gather per half-sweep, and the
    early-exit test (quirk Q3: the ROW factors, twice) one all-reduce(max).  Every entry is divided by the same factors in the
    same order as in the single-process sweep, so the scaled shards equal the shards of the scaled matrix bit for bit."""
    (rp, ci, va), (t_rp, t_ci, t_va) = K_blk, KT_blk
    dev, dt = va.device, va.dtype
    p = lambda t: t.data_ptr()
    world = 1 if comm is None else comm.world
    m_full, n_full = rows_K * world, rows_KT * world            # (equal, padded blocks)
    rn_full = torch.empty(m_full, dtype=dt, device=dev)
    cn_full = torch.empty(n_full, dtype=dt, device=dev)
    rn, cn = rn_full[r0:r0 + rows_K], cn_full[c0:c0 + rows_KT]
    work = torch.zeros(1, dtype=torch.float64, device=dev)
    nnz_K, nnz_KT = int(va.numel()), int(t_va.numel())
    sweeps = 0
    tstream = torch.cuda.current_stream(dev)
    for _ in range(int(max_iter)):
        with N.trace_range(f"pdlp: Ruiz sweep {sweeps + 1}", tstream):
            sweeps += 1
            N.check(lib.pdlp_csr_row_scale_factors(code, rows_K, p(rp), p(va), float(eps), p(rn), stream), "row factors")            # :49-50
            N.check(lib.pdlp_vec_muldiv(code, rows_K, p(D_row), p(rn), 1, stream), "D_row /= r")                                     # :51
            N.check(lib.pdlp_csr_div_rows(code, rows_K, p(rp), p(va), p(rn), stream), "K rows /= r")                                 # :52
            if comm is not None:
                comm.all_gather(rn_full)
            N.check(lib.pdlp_csr_div_cols(code, nnz_KT, p(t_ci), p(t_va), p(rn_full), stream), "K' cols /= r")
            N.check(lib.pdlp_csr_row_scale_factors(code, rows_KT, p(t_rp), p(t_va), float(eps), p(cn), stream), "col factors")       # :54-55
            N.check(lib.pdlp_vec_muldiv(code, rows_KT, p(D_col), p(cn), 1, stream), "D_col /= c")                                    # :56
            N.check(lib.pdlp_csr_div_rows(code, rows_KT, p(t_rp), p(t_va), p(cn), stream), "K' rows /= c")                           # :57
            if comm is not None:
                comm.all_gather(cn_full)
            N.check(lib.pdlp_csr_div_cols(code, nnz_K, p(ci), p(va), p(cn_full), stream), "K cols /= c")
            dev_from_one = C.c_double(0)
            N.check(lib.pdlp_vec_max_dev_from_one(code, rows_K, p(rn), p(work), C.byref(dev_from_one), stream), "max|1-r|")          # :60-61
            worst = dev_from_one.value
            if comm is not None:
                w = torch.tensor([worst], dtype=torch.float64, device=dev)
                comm.all_reduce_max(w)
                worst = float(w)
            if worst < eps:
                break
    return sweeps


def pock_chambolle_pass(lib, code, stream, rows_K, rows_KT, K_blk, KT_blk, D_row, D_col):
    """One Pock-Chambolle pass with alpha = 1 (PDLP's second scaling step) on the two CSR copies that ``_sweeps`` has equilibrated, in
    place: ``r_i = sqrt(sum_j |Ks_ij|)``, ``c_j = sqrt(sum_i |Ks_ij|)`` (1 where the sum is 0), both of the SAME matrix -- before either
    division, unlike a Ruiz sweep, whose column factors see the rows already divided -- then ``Ks <- diag(1/r) Ks diag(1/c)``,
    ``D_row /= r``, ``D_col /= c``.  The column factors are the row factors of the K' copy.  One process only: ``K_blk`` / ``KT_blk``
    are the whole copies (the sharded pass would need the sweeps' gather of the full factor vectors).  Returns ``(r, c)``."""
    (rp, ci, va), (t_rp, t_ci, t_va) = K_blk, KT_blk
    dev, dt = va.device, va.dtype
    p = lambda t: t.data_ptr()
    rn = torch.empty(rows_K, dtype=dt, device=dev)
    cn = torch.empty(rows_KT, dtype=dt, device=dev)
    nnz_K, nnz_KT = int(va.numel()), int(t_va.numel())
    with N.trace_range("pdlp: Pock-Chambolle pass", torch.cuda.current_stream(dev)):
        N.check(lib.pdlp_csr_row_l1_factors(code, rows_K, p(rp), p(va), p(rn), stream), "row 1-norm factors")
        N.check(lib.pdlp_csr_row_l1_factors(code, rows_KT, p(t_rp), p(t_va), p(cn), stream), "col 1-norm factors")
        N.check(lib.pdlp_vec_muldiv(code, rows_K, p(D_row), p(rn), 1, stream), "D_row /= r")
        N.check(lib.pdlp_csr_div_rows(code, rows_K, p(rp), p(va), p(rn), stream), "K rows /= r")
        N.check(lib.pdlp_csr_div_cols(code, nnz_KT, p(t_ci), p(t_va), p(rn), stream), "K' cols /= r")
        N.check(lib.pdlp_vec_muldiv(code, rows_KT, p(D_col), p(cn), 1, stream), "D_col /= c")
        N.check(lib.pdlp_csr_div_rows(code, rows_KT, p(t_rp), p(t_va), p(cn), stream), "K' rows /= c")
        N.check(lib.pdlp_csr_div_cols(code, nnz_K, p(ci), p(va), p(cn), stream), "K cols /= c")
    return rn, cn


@dataclass
class Scaling:
    """The factors of an equilibration, ``Ks = diag(D_row) K diag(D_col)``, and the one place where vectors are scaled by them and
    iterates un-scaled.  ``d_col`` / ``d_row``: ``(len,)`` for a shared matrix, ``(len, B)`` for a matrix per LP.  ``sweeps``: the
    Ruiz sweeps run; ``seconds``: the equilibration alone (no vector is scaled in them)."""
    d_col: torch.Tensor
    d_row: torch.Tensor
    sweeps: int = 0
    seconds: float = 0.0

    @staticmethod
    def _by(v, D, op):
        """``op(v, D)`` broadcast over the LPs: ``v`` None (passed on), ``(len,)``, ``(len, 1)`` or ``(len, B)``; a 2-D ``v`` on another
        device (a streamed family's host-resident columns) is scaled where it lives.  One LP's vector on the HIP device goes through
        ``pdlp_vec_muldiv`` on a clone: the same bits as torch's ``*`` and ``/``, whose kernels such a process then need not load"""
        if v is None:
            return None
        if v.is_cuda and v.shape == D.shape and v.dim() == 1 and v.dtype == D.dtype and D.is_contiguous():
            v = v.clone(memory_format=torch.contiguous_format)
            stream = torch.cuda.current_stream(v.device).cuda_stream
            N.check(N.load().pdlp_vec_muldiv(_DT[v.dtype], v.numel(), v.data_ptr(), D.data_ptr(), int(op is torch.div), stream), "v *|/= D")
            return v
        if v.dim() == 2:
            D = D.to(v.device).reshape(D.shape[0], -1)
        elif D.dim() == 2:
            v = v.view(-1, 1)
        return op(v, D)

    def scale(self, c, q, l, u, q_upper=None, quad_diag=None, quad_matrix=None):
        """``c * D_col, q * D_row, l / D_col, u / D_col`` as new tensors (enhancements.py:64-67); with ``q_upper`` (two-sided rows) a fifth,
        ``q_upper * D_row``: the other side of the same rows (``+inf`` stays ``+inf``, the factors are positive); with ``quad_diag``
        (the diagonal ``d`` of a quadratic objective) one more trailing value, ``d * D_col^2``: with ``x = D_col x_s`` the term
        ``1/2 d x^2`` is ``1/2 (d D_col^2) x_s^2`` (the factors themselves stay functions of K alone); with ``quad_matrix`` (the matrix
        ``Q`` of a quadratic objective, anything ``CsrPair.from_any`` takes) the last value is ``D_col Q D_col`` as a new ``CsrPair``:
        ``1/2 x'Qx = 1/2 x_s'(D_col Q D_col) x_s``.  Entry (i, j) is ``Q_ij (D_col_i D_col_j)`` -- the product of the two factors
        first, which commutes -- so a symmetric ``Q`` stays symmetric bit for bit."""
        by, mul, div = self._by, torch.mul, torch.div
        out = by(c, self.d_col, mul), by(q, self.d_row, mul), by(l, self.d_col, div), by(u, self.d_col, div)
        if q_upper is not None:
            out = out + (by(q_upper, self.d_row, mul),)
        if quad_diag is not None:
            out = out + (by(by(quad_diag, self.d_col, mul), self.d_col, mul),)
        return out if quad_matrix is None else out + (self._scale_quad_matrix(quad_matrix),)

    def _scale_quad_matrix(self, Q) -> CsrPair:
        d = self.d_col.reshape(-1)
        Qp = CsrPair.from_any(Q, device=d.device, dtype=d.dtype)
        rows_of = lambda rp: torch.repeat_interleave(torch.arange(Qp.n, device=d.device), rp[1:] - rp[:-1])
        val = Qp.val * (d[rows_of(Qp.rowptr)] * d[Qp.colidx.long()])
        t_val = Qp.t_val * (d[rows_of(Qp.t_rowptr)] * d[Qp.t_colidx.long()])
        return CsrPair(Qp.m, Qp.n, Qp.rowptr, Qp.colidx, val, Qp.t_rowptr, Qp.t_colidx, t_val)

    def unscale_x(self, x):
        """``D_col x`` (pdhg.py:161), the factors in the iterate's dtype"""
        return self._by(x, self.d_col.to(x.dtype), torch.mul)

    def unscale_y(self, y):
        """``D_row y`` (pdhg.py:162)"""
        return self._by(y, self.d_row.to(y.dtype), torch.mul)


def equilibrate(K_blk, KT_blk, *, comm=None, r0=0, c0=0, max_iter=20, eps=1e-6, pock_chambolle=False) -> Scaling:
    """The one body of every preconditioner here: the Ruiz sweeps (enhancements.py:45-62; early exit on the ROW factors twice, quirk
    Q3) and, with ``pock_chambolle`` (not in the reference), one ``pock_chambolle_pass`` composed into the same factors, IN PLACE on
    the CSR triples ``K_blk`` / ``KT_blk``: the whole copies of K and K', or with ``comm`` this rank's equal padded row blocks of them,
    which start at row ``r0`` resp. ``c0``.  Returns the factors of these rows of K and of K' (local blocks when sharded)."""
    t0 = time.time()
    comm = comm if comm is not None and comm.world > 1 else None
    if pock_chambolle and comm is not None:
        raise ValueError("pock_chambolle has no sharded form yet (the pass needs the sweeps' gather of the full factor vectors)")
    dev, dt = K_blk[2].device, K_blk[2].dtype
    if dev.type != "cuda":
        raise N.PdlpError("the equilibration runs on the HIP device (there is no CPU fallback)")
    lib, code = N.load(), _DT[dt]
    stream = torch.cuda.current_stream(dev)
    rows_K, rows_KT = int(K_blk[0].numel()) - 1, int(KT_blk[0].numel()) - 1
    D_row = torch.ones(rows_K, dtype=dt, device=dev)
    D_col = torch.ones(rows_KT, dtype=dt, device=dev)
    sweeps = _sweeps(lib, code, stream.cuda_stream, rows_K, rows_KT, K_blk, KT_blk, D_row, D_col, max_iter, eps, comm, r0, c0)
    if pock_chambolle:
        pock_chambolle_pass(lib, code, stream.cuda_stream, rows_K, rows_KT, K_blk, KT_blk, D_row, D_col)
    stream.synchronize()
    return Scaling(D_col, D_row, sweeps, time.time() - t0)


def equilibrate_matrix(K, device=None, max_iter=20, eps=1e-6, pock_chambolle=False):
    """``(Ks, Scaling)`` of a matrix alone: ``Ks`` a new ``CsrPair`` with both copies scaled consistently; the caller's ``K`` (dense /
    COO / scipy sparse / ``CsrPair``) is left as it is.  ``device`` None: the current HIP device."""
    Ks = CsrPair.from_any(K, device=resolve_device(device)).clone()
    return Ks, equilibrate((Ks.rowptr, Ks.colidx, Ks.val), (Ks.t_rowptr, Ks.t_colidx, Ks.t_val), max_iter=max_iter, eps=eps,
                           pock_chambolle=pock_chambolle)


def ruiz_precondition_shard(shard: dict, comm, max_iter=20, eps=1e-6) -> dict:
    """Ruiz on a problem that only exists as shards: ``shard`` = this rank's keyword arguments of ``PdlpEngine`` as
    ``distributed.shard_arrays`` / ``gen_lp_shard_arrays`` build them (row block of K and of K' in the padded layout, local
    ``c, q, l, u``).  Returns a new dict with the scaled blocks and vectors plus ``d_col`` / ``d_row`` (local blocks) -- no rank
    ever holds a full matrix.  ``shard["ruiz_seconds"]`` / ``["ruiz_sweeps"]`` record the cost.  (enhancements.py:4-71)"""
    t0 = time.time()
    (rp, ci, va), (t_rp, t_ci, t_va) = shard["K_rows"], shard["KT_rows"]
    dev, dt = va.device, va.dtype
    if dev.type != "cuda":
        raise N.PdlpError("ruiz_precondition_shard runs on the HIP device (there is no CPU fallback)")
    (r0, r1), (c0, c1) = shard["rows"], shard["cols"]
    ml, nl = r1 - r0, c1 - c0
    world = 1 if comm is None else comm.world
    if ml * world != shard["m"] or nl * world != shard["n"]:
        raise ValueError("sharded Ruiz needs the equal, padded blocks of torchpdlp_amd/distributed.py")
    idx = lambda t, it: t.to(device=dev, dtype=it).contiguous()
    K_blk = (idx(rp, torch.int64), idx(ci, torch.int32), va.clone())
    KT_blk = (idx(t_rp, torch.int64), idx(t_ci, torch.int32), t_va.to(dev).clone())
    scaling = equilibrate(K_blk, KT_blk, comm=comm, r0=r0, c0=c0, max_iter=max_iter, eps=eps)
    vec = lambda v, ln: as_vec(v, ln, dev, dt)
    c_s, q_s, l_s, u_s = scaling.scale(vec(shard["c"], nl), vec(shard["q"], ml), vec(shard["l"], nl), vec(shard["u"], nl))
    torch.cuda.current_stream(dev).synchronize()
    out = dict(shard)
    out.update(K_rows=K_blk, KT_rows=KT_blk, c=c_s, q=q_s, l=l_s, u=u_s, d_col=scaling.d_col, d_row=scaling.d_row,
               ruiz_seconds=time.time() - t0, ruiz_sweeps=scaling.sweeps)
    return out


def ruiz_precondition(c, K, q, l, u, device=None, max_iter=20, eps=1e-6, pock_chambolle=False, q_upper=None, quad_diag=None,
                      quad_matrix=None):
    """Returns ``(K_s, c_s, q_s, l_s, u_s, (D_col, D_row, K, c, q, l, u), time_used)`` like the reference: ``equilibrate_matrix``
    (``K_s`` a ``CsrPair``) and ``Scaling.scale`` of the four vectors, as ``(len, 1)`` columns.  With ``q_upper`` (two-sided rows) the
    scaled ``q_upper`` follows ``u_s`` in the result, with ``quad_diag`` (quadratic objective) the scaled diagonal comes after it, and
    with ``quad_matrix`` the scaled matrix ``D_col Q D_col`` (a ``CsrPair``) after that."""
    t0 = time.time()
    Ks, scaling = equilibrate_matrix(K, device, max_iter, eps, pock_chambolle)
    vec = lambda v, ln: as_vec(v, ln, Ks.device, Ks.dtype)
    scaled = scaling.scale(vec(c, Ks.n), vec(q, Ks.m), vec(l, Ks.n), vec(u, Ks.n), None if q_upper is None else vec(q_upper, Ks.m),
                           None if quad_diag is None else vec(quad_diag, Ks.n))
    torch.cuda.current_stream(Ks.device).synchronize()
    if quad_matrix is not None:
        scaled = scaled + (scaling._scale_quad_matrix(quad_matrix),)
    col = lambda v: v.view(-1, 1) if isinstance(v, torch.Tensor) else v
    return (Ks, *map(col, scaled), (col(scaling.d_col), col(scaling.d_row), K, c, q, l, u), time.time() - t0)


def ruiz_precondition_batch(K, K_values, device=None, max_iter=20, eps=1e-6, pock_chambolle=False):
    """``equilibrate_matrix`` of every LP's matrix of a batch over one pattern: ``K`` (a ``CsrPair``) gives the pattern, column b of
    ``K_values`` ``(nnz, B)`` the values of LP b in its CSR order.  A host loop over the LPs (set-up, once per solve).  Returns
    ``(Ks_values (nnz, B), KsT_values (nnz, B) in the order of K', D_col (n, B), D_row (m, B), seconds)``."""
    t0 = time.time()
    Kp = CsrPair.from_any(K, device=device)
    vals = K_values.to(device=Kp.device, dtype=Kp.dtype)
    perm = Kp.transpose_perm()
    sv, stv, dc, dr = [], [], [], []
    for b in range(vals.shape[1]):
        Ks, scaling = equilibrate_matrix(Kp.with_values(vals[:, b].contiguous(), perm), Kp.device, max_iter, eps, pock_chambolle)
        sv.append(Ks.val); stv.append(Ks.t_val); dc.append(scaling.d_col); dr.append(scaling.d_row)
    st = lambda cols: torch.stack(cols, dim=1).contiguous()
    return st(sv), st(stv), st(dc), st(dr), time.time() - t0
