"""PdlpEngine: one LP (or one rank's shard of it) resident on one MI355X, driven through the C ABI.

torch is used for storage (problem arrays, one workspace tensor) and, when the problem is sharded
over several GPUs, for the collectives between the half-steps (``torch.distributed`` backend
``nccl`` = RCCL over xGMI).  All arithmetic of the hot path happens in ``libpdlp_hip.so``.

One class over three files, cut like the library's host code: construction, workspace, state, ``iterate`` and the KKT / report /
restart / infeasibility / population wrappers here; which kernel multiplies each matrix in ``engine_kernels.py``; what only sharded
engines need in ``engine_exchange.py`` (the collectives themselves: ``comm.py``).
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from typing import Optional, Tuple

import torch

from . import _native as N
from .comm import Comm                                          # noqa: F401  (imported from here by the package, tests and tools)
from .engine_exchange import Exchange
from .engine_kernels import KernelChoice
from .sparse import CsrPair, as_vec

_DT = {torch.float32: N.PDLP_F32, torch.float64: N.PDLP_F64}
# the buffers that hold x and y of the current iterate, the average and the previous iterate
_ITERATE_BUFFERS = {N.CUR: (N.BUF_X_CUR, N.BUF_Y_CUR), N.AVG: (N.BUF_X_AVG, N.BUF_Y_AVG), N.PREV: (N.BUF_X_PREV, N.BUF_Y_PREV)}


def values_are_float32(val: torch.Tensor) -> bool:
    """every entry of a float64 array is a float32 number (so the matrix can be held in float32 without changing the LP)"""
    return val.dtype == torch.float32 or bool((val.float().to(val.dtype) == val).all())


def exportable_bytes(nbytes: int) -> int:
    """size of a device allocation that can hold ``nbytes`` AND be opened by another process: a multiple of 2 MB (what torch's
    allocator makes of a large request anyway) without bit 31 -- hipIpcOpenMemHandle never returns for 2-4 GiB, 6-8 GiB, ... on
    ROCm 7.2 (tools/ipc_torch_probe.py) -- i.e. such sizes go up to the next multiple of 4 GiB"""
    size = -(-int(nbytes) // (2 << 20)) * (2 << 20)
    if size & 0x80000000:
        size = (size | 0xFFFFFFFF) + 1
    return size


Knobs = namedtuple("Knobs", "running_kkt kty_reuse begin_inline producer_pieces graph exchange_chunks delta lib_comm tiled sorted "
                            "tile_lw tile_rpt tile_groups peer_trace")


def knobs_from_env(env=None) -> Knobs:
    """The ``PDLP_*`` test / tool switches of an engine, read once when it is constructed (the library reads no environment: what
    concerns the handle goes through ``pdlp_set_option``).  Variable, default, what it maps to ("0..": first character 0):

    PDLP_RUNNING_KKT      on     "0..": ``OPT_RUNNING_KKT`` = 0
    PDLP_NO_KTY_REUSE     unset  set to anything, the empty string included: ``OPT_KTY_REUSE`` = 0
    PDLP_BEGIN_INLINE     on     "0..": a sharded engine leaves ``OPT_BEGIN_INLINE`` at 0
    PDLP_PRODUCER_PIECES  on     "0..": ``OPT_PRODUCER_PIECES`` = 0 (``set_producer_pieces``)
    PDLP_GRAPH            unset  set to anything: ``OPT_GRAPH`` = 1 on an engine that is not sharded
    PDLP_EXCHANGE_CHUNKS  1      an integer > 1: ``set_exchange_chunks`` on a sharded engine that may tile
    PDLP_DELTA            on     "0" exactly: a mixed-precision engine built with ``delta=None`` stays out of delta mode
    PDLP_LIB_COMM         off    "1" exactly: ``enable_library_comm()`` at construction (RCCL backend, an engine that may tile)
    PDLP_TILED            auto   0 / 1 / auto / time: the mode of ``engine_kernels.wants_tiles``
    PDLP_SORTED           auto   1: column-sorted row blocks for every matrix; 0: never; else for clustered matrices, if they pay
    (PDLP_PACKED_ITEMS is not one of these: ``engine_kernels.packed_items_mode`` reads it whenever tiles are attached, so that one
    process can alternate the two index streams engine by engine.)
    PDLP_TILE_LW, PDLP_TILE_RPT, PDLP_TILE_GROUPS  unset  integers (empty = unset): ``build_tiles(lw=, rpt=, groups=)``
    PDLP_PEER_TRACE       unset  non-empty: ``enable_peer_exchange`` reports its progress on stderr

    (``PDLP_LIB`` and ``PDLP_ROCTX`` belong to ``_native.py``.)"""
    env = os.environ if env is None else env
    first_not_0 = lambda name: env.get(name, "1")[:1] != "0"
    number = lambda name: int(env[name]) if env.get(name) else None
    return Knobs(first_not_0("PDLP_RUNNING_KKT"), env.get("PDLP_NO_KTY_REUSE") is None, first_not_0("PDLP_BEGIN_INLINE"),
                 first_not_0("PDLP_PRODUCER_PIECES"), env.get("PDLP_GRAPH") is not None, int(env.get("PDLP_EXCHANGE_CHUNKS", "1")),
                 env.get("PDLP_DELTA", "1") != "0", env.get("PDLP_LIB_COMM", "0") == "1", env.get("PDLP_TILED", "auto"),
                 env.get("PDLP_SORTED", "auto"), number("PDLP_TILE_LW"), number("PDLP_TILE_RPT"), number("PDLP_TILE_GROUPS"),
                 bool(env.get("PDLP_PEER_TRACE")))


class PdlpEngine(KernelChoice, Exchange):
    """Device-resident restarted-PDHG state for one LP shard.

    Parameters are this rank's blocks: ``K_rows`` = CSR of rows [row0,row1) of K, ``KT_rows`` = CSR of
    rows [col0,col1) of K' (global indices), ``c,l,u`` of length col1-col0, ``q`` of length row1-row0.
    """

    def __init__(self, m: int, n: int, m_ineq: int, K_rows, KT_rows, c, q, l, u, rows: Tuple[int, int] = None,
                 cols: Tuple[int, int] = None, d_col=None, d_row=None, comm: Optional[Comm] = None, vec_dtype=None,
                 delta: Optional[bool] = None, exact=None, tiles: bool = True, q_upper=None, quad_diag=None, quad_matrix=None):
        """``q_upper`` (length row1-row0, or None): two-sided rows ``q <= K x <= q_upper`` on the inequality rows (``set_row_upper``).
        ``quad_diag`` (length n, or None): the objective ``c'x + 1/2 sum_j d_j x_j^2`` (``set_objective_diag``).
        ``quad_matrix`` (n x n, symmetric positive semidefinite, or None): the objective ``c'x + 1/2 x'Qx`` (``set_objective_matrix``).
        ``vec_dtype=torch.float64`` over float32 matrix values selects the mixed precision (``PDLP_MIXED``): float64 vectors,
        products and sums on a float32 matrix (12 -> 8 bytes per non-zero); ``delta`` (default: ``PDLP_DELTA`` in the environment,
        else on) then runs the iterations on the float32 kernels over float32 difference vectors added to float64 anchor
        products (``pdlp_set_delta`` in include/pdlp_hip.h).  ``exact`` = ``(K_rows, KT_rows)`` in float64: the TRUE matrix when the
        float32 one handed in as ``K_rows`` / ``KT_rows`` is only its rounding (any float64 matrix, a Ruiz-scaled one): the anchors
        of delta mode are then evaluated with it (a second, float64 CSR handle over the same row blocks; ``pdlp_set_anchors``).
        A scaled matrix whose entries ARE float32 numbers (Ruiz on a +-1 matrix is the identity) needs no ``exact``."""
        self.lib = N.load()
        N.trace_range.enabled()                # (PDLP_ROCTX=1|2: roctx ranges for rocprofv3 --marker-trace; once per process)
        rows = (0, m) if rows is None else rows
        cols = (0, n) if cols is None else cols
        self.m, self.n, self.m_ineq = int(m), int(n), int(m_ineq)
        self.rows, self.cols = (int(rows[0]), int(rows[1])), (int(cols[0]), int(cols[1]))
        self.ml, self.nl = self.rows[1] - self.rows[0], self.cols[1] - self.cols[0]
        self.comm = comm if (comm is not None and comm.world > 1) else None
        if self.comm is None and (self.ml != self.m or self.nl != self.n):
            raise ValueError("a sharded problem needs a communicator")
        val = K_rows[2]
        self.device, self.mat_dtype = val.device, val.dtype
        self.dtype = self.mat_dtype if vec_dtype is None else vec_dtype       # the working precision: vectors, sums, scalars
        if self.device.type != "cuda":
            raise N.PdlpError("PdlpEngine needs the problem on a HIP device (there is no CPU fallback)")
        if self.mat_dtype not in _DT or self.dtype not in _DT:
            raise ValueError(f"unsupported dtype {self.mat_dtype} / {self.dtype}")
        self.mixed = self.dtype != self.mat_dtype
        if self.mixed and (self.mat_dtype, self.dtype) != (torch.float32, torch.float64):
            raise ValueError("mixed precision means float32 matrix values under float64 vectors")
        if exact is not None and not self.mixed:
            raise ValueError("`exact` (the float64 matrix behind a float32 rounding) belongs to mixed precision")
        i32 = lambda t: t.to(device=self.device, dtype=torch.int32).contiguous()
        i64 = lambda t: t.to(device=self.device, dtype=torch.int64).contiguous()        # row pointers: 64-bit in the ABI
        fv = lambda t, ln: None if t is None else as_vec(t, ln, self.device, self.dtype)
        # keep every tensor the library points into alive
        self.K = (i64(K_rows[0]), i32(K_rows[1]), K_rows[2].to(self.mat_dtype).contiguous())
        self.KT = (i64(KT_rows[0]), i32(KT_rows[1]), KT_rows[2].to(self.device, self.mat_dtype).contiguous())
        self.c, self.l, self.u = fv(c, self.nl), fv(l, self.nl), fv(u, self.nl)
        self.q = fv(q, self.ml)
        self.d_col, self.d_row = fv(d_col, self.nl), fv(d_row, self.ml)
        self.stream = torch.cuda.current_stream(self.device)
        ptr = lambda t: None if t is None else t.data_ptr()
        self.prob = N.PdlpProblem(N.PDLP_MIXED if self.mixed else _DT[self.dtype], self.device.index or 0, self.m, self.n, self.m_ineq,
                                  self.rows[0], self.rows[1], self.cols[0], self.cols[1],
                                  ptr(self.K[0]), ptr(self.K[1]), ptr(self.K[2]),
                                  ptr(self.KT[0]), ptr(self.KT[1]), ptr(self.KT[2]),
                                  ptr(self.c), ptr(self.l), ptr(self.u), ptr(self.q), ptr(self.d_col), ptr(self.d_row),
                                  self.stream.cuda_stream)
        nbytes = C.c_int64(0)
        N.check(self.lib.pdlp_workspace_bytes(C.byref(self.prob), C.byref(nbytes)), "pdlp_workspace_bytes")
        self.workspace = self._alloc_workspace(int(nbytes.value) + 256, exportable=comm is not None)
        self._ws_off = (-self.workspace.data_ptr()) % 256
        self.h = N._H()
        N.check(self.lib.pdlp_create(C.byref(self.h), C.byref(self.prob), self.workspace.data_ptr() + self._ws_off,
                                     nbytes.value), "pdlp_create")
        self._views = {}
        self._want_tiles = bool(tiles)
        self.q_upper = None
        if q_upper is not None:
            self.set_row_upper(q_upper)
        self.quad_diag = None
        if quad_diag is not None:
            self.set_objective_diag(quad_diag)
        self.quad_matrix = self._quad_work = None
        if quad_matrix is not None:
            self.set_objective_matrix(quad_matrix)
        # test / tool knobs of the handle (knobs_from_env)
        kn = self.knobs = knobs_from_env()
        if not kn.running_kkt:
            self.set_option(N.OPT_RUNNING_KKT, 0)
        if not kn.kty_reuse:
            self.set_option(N.OPT_KTY_REUSE, 0)
        if self.comm is not None and kn.begin_inline:
            # the torch.distributed loop issues every exchange asynchronously BEFORE it starts the next product on the own block
            # (_iterate_loop): the local panels then go onto the handle's stream, no side stream / events (pdlp_hip.h, PDLP_OPT_BEGIN_INLINE)
            self.set_option(N.OPT_BEGIN_INLINE, 1)
        self.producer_pieces = kn.producer_pieces
        if not self.producer_pieces:
            self.set_option(N.OPT_PRODUCER_PIECES, 0)
        if kn.graph and self.comm is None and self.quad_matrix is None:      # (no replay with a sparse quadratic objective)
            self.set_option(N.OPT_GRAPH, 1)
        self.exact = None
        if exact is not None:          # the true float64 matrix, CSR kernels only: two products per restart
            self.exact = PdlpEngine(m, n, m_ineq, exact[0], exact[1], c, q, l, u, rows=rows, cols=cols, d_col=d_col, d_row=d_row,
                                    comm=comm, tiles=False)       # (d_col / d_row: the un-scaled solution report)
        self._sorted = [None, None]
        self._mv_work = {}
        self.xchunks, self._plans = 1, {}
        self.tiles = [None, None]
        self.kernels = ["csr", "csr"]
        self._maybe_attach_tiles()
        if self.comm is not None and tiles and kn.exchange_chunks > 1:
            self.set_exchange_chunks(kn.exchange_chunks)
        self.delta = False
        if self.mixed and (delta if delta is not None else kn.delta):
            self.set_delta(True)
        # the exchange inside the library (one C call per restart period) is opt-in: PDLP_LIB_COMM=1 here, or
        # enable_library_comm() by the caller (bench.py does); the default is the torch.distributed loop
        self.lib_comm, self.lib_comm_log = False, []
        self.peer_on, self.peer_log, self.peer_local_first = False, [], False     # direct exchange over HIP IPC (enable_peer_exchange)
        self.peer_push, self.peer_form = False, 0
        if self.comm is not None and self.comm.backend == "nccl" and tiles and kn.lib_comm:
            self.enable_library_comm()

    def set_option(self, option: int, value: int):
        """``pdlp_set_option``: the handle's test / tool switches (``N.OPT_*``)"""
        N.check(self.lib.pdlp_set_option(self.h, int(option), int(value)), "pdlp_set_option")

    def set_row_upper(self, q_upper):
        """Two-sided rows (``pdlp_set_row_upper``, include/pdlp_hip.h): ``q_i <= (K x)_i <= q_upper_i`` on the inequality rows, ``+inf``
        = a one-sided row; ``y_i > 0``: the lower side is active, ``y_i < 0``: the upper side.  ``None`` switches them off.  Validated
        here (``ranged.check_row_upper``: ``ValueError``); float32 / float64 engines on one GPU (``ValueError`` otherwise).  While set,
        ``detect_infeasibility`` and the population calls raise ``PdlpError``."""
        from . import compose, ranged
        if q_upper is None:
            N.check(self.lib.pdlp_set_row_upper(self.h, None), "pdlp_set_row_upper")
            self.q_upper = None
            return
        compose.check_composition(q_upper=True, mixed=self.mixed, comm=self.comm is not None)
        qu = ranged.check_row_upper(self.q, as_vec(q_upper, self.ml, self.device, self.dtype), self.m_ineq)
        N.check(self.lib.pdlp_set_row_upper(self.h, qu.data_ptr()), "pdlp_set_row_upper")
        self.q_upper = qu                      # (kept alive: the library points into it)

    def set_objective_diag(self, d):
        """Diagonal quadratic objective (``pdlp_set_objective_diag``, include/pdlp_hip.h): ``min c'x + 1/2 sum_j d_j x_j^2`` with
        ``d >= 0`` of length n, in the engine's scaling when it has one (``Scaling.scale(..., quad_diag=)``: ``d D_col^2``).  ``None``
        switches the term off.  Validated here (``quad.check_quad_diag``: ``ValueError``); float32 / float64 engines on one GPU --
        the library refuses the others (``PdlpError``).  While set, ``kkt`` / ``report`` give the quadratic problem's objectives
        (``p = c'x + 1/2 x'Dx``, ``d_adj`` with ``-1/2 x'Dx``) and reduced costs ``project_lambda_box(c + Dx - K'y)``, and
        ``detect_infeasibility``, the population calls and the batch calls raise ``PdlpError``."""
        from .quad import check_quad_diag
        if d is None:
            N.check(self.lib.pdlp_set_objective_diag(self.h, None), "pdlp_set_objective_diag")
            self.quad_diag = None
            return
        d = as_vec(check_quad_diag(d, self.nl), self.nl, self.device, self.dtype)
        N.check(self.lib.pdlp_set_objective_diag(self.h, d.data_ptr()), "pdlp_set_objective_diag")
        self.quad_diag = d                     # (kept alive: the library points into it)

    def set_objective_matrix(self, Q):
        """Sparse quadratic objective (``pdlp_set_objective_matrix``, include/pdlp_hip.h): ``min c'x + 1/2 x'Qx`` with ``Q`` n x n,
        symmetric and positive semidefinite (the caller's duty), in the engine's scaling when it has one (``Scaling.scale(...,
        quad_matrix=)``: ``D_col Q D_col``).  ``None`` takes it away.  Validated here (``quad.check_quad_matrix``: ``ValueError``);
        float32 / float64 engines on one GPU without graph replay -- the library refuses the others (``PdlpError``).  While set,
        ``iterate`` takes the linearised step (fixed step only; the caller keeps ``rules.qp_eta``) and ``objective_iterate`` the same
        step under its own adaptive rule, ``kkt`` / ``report`` give the quadratic problem's objectives (``p = c'x + 1/2 x'Qx``,
        ``d_adj`` with ``-1/2 x'Qx``) and reduced costs ``project_lambda_box(c + Qx - K'y)``, and the LP's adaptive step
        (``iterate(n, True)``), ``halpern_iterate``, ``detect_infeasibility``, the population calls and the batch calls raise
        ``PdlpError``."""
        from .quad import check_quad_matrix
        if Q is None:
            N.check(self.lib.pdlp_set_objective_matrix(self.h, None, None, None, None, 0), "pdlp_set_objective_matrix")
            self.quad_matrix = self._quad_work = None
            return
        Qp = check_quad_matrix(Q, self.n).to(device=self.device, dtype=self.dtype)
        nbytes = C.c_int64(0)
        N.check(self.lib.pdlp_objective_matrix_bytes(self.h, Qp.nnz, C.byref(nbytes)), "pdlp_objective_matrix_bytes")
        work = torch.empty(int(nbytes.value) + 256, dtype=torch.uint8, device=self.device)
        off = (-work.data_ptr()) % 256
        # (a Q without stored entries: its empty arrays have no address, and NULL means "take Q away" -- one unused element each)
        ci = Qp.colidx if Qp.nnz else torch.zeros(1, dtype=torch.int32, device=self.device)
        va = Qp.val if Qp.nnz else torch.zeros(1, dtype=self.dtype, device=self.device)
        N.check(self.lib.pdlp_set_objective_matrix(self.h, Qp.rowptr.data_ptr(), ci.data_ptr(), va.data_ptr(),
                                                   work.data_ptr() + off, nbytes.value), "pdlp_set_objective_matrix")
        self.quad_matrix, self._quad_work = Qp, (work, ci, va)        # (kept alive: the library points into all of them)

    def objective_product(self, x_full: torch.Tensor) -> torch.Tensor:
        """``Q x`` (``pdlp_objective_product``): the plain product over the matrix of ``set_objective_matrix``"""
        x = as_vec(x_full, self.n, self.device, self.dtype)
        out = torch.empty(self.nl, dtype=self.dtype, device=self.device)
        N.check(self.lib.pdlp_objective_product(self.h, x.data_ptr(), out.data_ptr()), "pdlp_objective_product")
        return out

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        th = getattr(self, "_comm_init_thread", None)
        if h and th is not None and th.is_alive():
            # a pdlp_comm_init that timed out is still inside ncclCommInitRank with this handle: destroying it now would race with
            # that thread (it may yet write the communicator, the stream and the events).  The handle is leaked on purpose; the
            # owner should end the process (bench.py does) rather than reuse it.
            return
        if h:
            self.lib.pdlp_destroy(h)
        if getattr(self, "_ws_pool", None) is not None:        # (the block goes back before its private pool does)
            self._views = {}
            self.workspace = None
            self._ws_pool = None

    @classmethod
    def from_full(cls, K: CsrPair, c, q, l, u, m_ineq: int, d_col=None, d_row=None, vec_dtype=None, delta=None,
                  exact: Optional[CsrPair] = None, q_upper=None, quad_diag=None, quad_matrix=None) -> "PdlpEngine":
        """single-GPU engine over a whole problem (``exact``: the float64 matrix of which ``K`` is the float32 rounding)"""
        ex = None if exact is None else ((exact.rowptr, exact.colidx, exact.val), (exact.t_rowptr, exact.t_colidx, exact.t_val))
        return cls(K.m, K.n, m_ineq, (K.rowptr, K.colidx, K.val), (K.t_rowptr, K.t_colidx, K.t_val), c, q, l, u,
                   d_col=d_col, d_row=d_row, vec_dtype=vec_dtype, delta=delta, exact=ex, q_upper=q_upper, quad_diag=quad_diag,
                   quad_matrix=quad_matrix)

    # ---- buffers ------------------------------------------------------------------------------------
    def buffer(self, which: int) -> torch.Tensor:
        """torch view of one of the library's device buffers (roles move: query again after a step)"""
        p = C.c_void_p()
        N.check(self.lib.pdlp_buffer_ptr(self.h, which, C.byref(p)), "pdlp_buffer_ptr")
        key = (p.value, which in (N.BUF_RED, N.BUF_SCALARS))
        v = self._views.get(key)
        if v is None:
            off = p.value - self.workspace.data_ptr()
            if which in (N.BUF_RED, N.BUF_SCALARS):
                cnt = N.NRED if which == N.BUF_RED else N.NSCAL
                v = self.workspace[off:off + cnt * 8].view(torch.float64)
            elif which in (N.BUF_GDX, N.BUF_GDY):
                v = self.workspace[off:off + (self.n if which == N.BUF_GDX else self.m) * 4].view(torch.float32)
            else:
                ln = {N.BUF_X_SUM: self.nl, N.BUF_Y_SUM: self.ml, N.BUF_DX: self.n, N.BUF_DY: self.m, N.BUF_LAM_PREV: self.nl}.get(
                    which, self.n if which <= N.BUF_X_AVG else self.m)
                v = self.workspace[off:off + ln * self.dtype.itemsize].view(self.dtype)
            self._views[key] = v
        return v

    def _alloc_workspace(self, nbytes: int, exportable: bool) -> torch.Tensor:
        """the handle's workspace.  Of a sharded engine it may be exported to the other ranks over HIP IPC (the direct exchange): it
        then gets an allocation OF ITS OWN (a private pool of torch's allocator: a block carved out of a cached segment drags the
        whole segment along) of a size that another process can open (``exportable_bytes``; pdlp_peer_export refuses any other)."""
        if not (exportable and self.device.type == "cuda" and hasattr(torch.cuda, "MemPool")):
            return torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._ws_pool = torch.cuda.MemPool()
        with torch.cuda.use_mem_pool(self._ws_pool, device=self.device):
            return torch.empty(exportable_bytes(nbytes), dtype=torch.uint8, device=self.device)

    def _gather(self, which: int):
        if self.comm is not None:
            self.comm.all_gather(self.buffer(which))

    def _reduce_sums(self):
        """the ranks' partial sums of the last ``*_local`` call, added up on every rank"""
        if self.comm is not None:
            self.comm.all_reduce_sum(self.buffer(N.BUF_RED))

    def _gather_iterate(self, which: int):
        """every rank's block of x and of y of the current iterate / the average / the previous iterate (nothing to do on one GPU)"""
        for b in _ITERATE_BUFFERS[which]:
            self._gather(b)

    def set_delta(self, on: bool):
        """delta mode of a mixed-precision engine (include/pdlp_hip.h, pdlp_set_delta)"""
        N.check(self.lib.pdlp_set_delta(self.h, int(bool(on))), "pdlp_set_delta")
        self.delta = bool(on)

    def delta_state(self) -> dict:
        out = (C.c_int32 * 3)()
        N.check(self.lib.pdlp_delta_state(self.h, out), "pdlp_delta_state")
        return dict(delta=bool(out[0]), anchors_valid=bool(out[1]), dy_folded=bool(out[2]))

    def refresh_products(self):
        """recompute K x and K'y of the current iterate exactly (float64 accumulation): the anchors of delta mode"""
        self._gather_iterate(N.CUR)        # (sharded: the products need the complete iterate)
        if self.exact is None:
            N.check(self.lib.pdlp_refresh_products(self.h), "pdlp_refresh_products")
            return
        # the handle's matrix is the float32 rounding of the true one: anchors from the true one
        x, y = (self.buffer(N.BUF_X_CUR), self.buffer(N.BUF_Y_CUR)) if self.comm is not None else self.get_iterate(N.CUR)
        kx, kty = self.exact.spmv(x, False), self.exact.spmv(y, True)
        N.check(self.lib.pdlp_set_anchors(self.h, kx.data_ptr(), kty.data_ptr()), "pdlp_set_anchors")

    def _ensure_anchors(self):
        """delta mode computes on anchors: make them valid where the library cannot do that by itself -- it needs the complete
        iterate (gathers) or the true matrix (``exact``).  The callers say when that is."""
        if self.delta and not self.delta_state()["anchors_valid"]:
            self.refresh_products()

    # ---- state --------------------------------------------------------------------------------------
    def set_iterate(self, x_local: torch.Tensor, y_local: torch.Tensor):
        x = as_vec(x_local, self.nl, self.device, self.dtype)
        y = as_vec(y_local, self.ml, self.device, self.dtype)
        N.check(self.lib.pdlp_set_iterate(self.h, x.data_ptr(), y.data_ptr()), "pdlp_set_iterate")
        self._gather_iterate(N.CUR)

    def get_iterate(self, which: int = N.CUR) -> Tuple[torch.Tensor, torch.Tensor]:
        x = torch.empty(self.nl, dtype=self.dtype, device=self.device)
        y = torch.empty(self.ml, dtype=self.dtype, device=self.device)
        N.check(self.lib.pdlp_get_iterate(self.h, which, x.data_ptr(), y.data_ptr()), "pdlp_get_iterate")
        return x, y

    def set_step(self, eta: float, omega: float, theta: float = 1.0, iteration: int = 0):
        N.check(self.lib.pdlp_set_step(self.h, float(eta), float(omega), float(theta), int(iteration)), "pdlp_set_step")

    def set_omega(self, omega: float):
        N.check(self.lib.pdlp_set_omega(self.h, float(omega)), "pdlp_set_omega")

    def scalars(self) -> dict:
        out = (C.c_double * N.NSCAL)()
        N.check(self.lib.pdlp_get_scalars(self.h, out), "pdlp_get_scalars")
        names = ("eta", "omega", "theta", "tau", "sigma", "w_pending", "eta_sum", "k", "inv1pt", "accepted", "eta_bar",
                 "denominator")
        return dict({k: out[i] for i, k in enumerate(names)}, curvature=out[N.S_CURV])

    # ---- iterations ---------------------------------------------------------------------------------
    def iterate(self, iters: int, adaptive: bool):
        """`iters` PDHG iterations, no host synchronisation (pdhg.py:76-112), by one of three drivers: ``pdlp_iterate`` -- on one
        GPU, with the exchange inside the library (RCCL) or with the direct exchange, which has no collective in it -- or, for a
        sharded engine without either, the torch.distributed loop (engine_exchange.py)."""
        iters = int(iters)
        self._peer_check()
        loop = self.comm is not None and not self.lib_comm and not self.peer_on
        # pdlp_iterate refreshes the anchors of delta mode by itself (on one GPU inside the first half-step, with the library's own
        # gathers when it has a communicator) -- unless they come from the true matrix or it runs the direct exchange, which may
        # not issue the gathers; the loop's half-steps are single calls that expect them valid
        if iters > 0 and (self.exact is not None or self.peer_on or loop):
            self._ensure_anchors()
        if loop:
            self._iterate_loop(iters, adaptive)
        else:
            N.check(self.lib.pdlp_iterate(self.h, iters, int(adaptive)), "pdlp_iterate")

    def objective_iterate(self, iters: int):
        """``iters`` adaptive iterations of the linearised step of an engine with ``quad_matrix`` (``pdlp_objective_iterate``,
        include/pdlp_hip.h), no host synchronisation: the step-size rule of ``iterate(iters, True)`` with the curvature ``dx'Q dx``
        measured along the step in its denominator, at the fixed step's three products per iteration.  ``scalars()`` reports the last
        iteration's ``"accepted"``, ``"eta_bar"``, ``"denominator"`` (``2 dy'K dx``) and ``"curvature"``.  ``flush_average(True)``,
        ``restart`` and ``set_omega`` as for an adaptive LP.  ``PdlpError`` without ``quad_matrix``."""
        N.check(self.lib.pdlp_objective_iterate(self.h, int(iters)), "pdlp_objective_iterate")

    def halpern_iterate(self, iters: int):
        """``iters`` iterations of the restarted, reflected Halpern iteration (``pdlp_halpern_iterate``, include/pdlp_hip.h), no host
        synchronisation: ``N.CUR`` is the Halpern iterate afterwards and ``N.AVG`` the candidate -- one fixed PDHG step from the
        iterate before the last iteration -- which ``kkt(N.AVG)`` evaluates and ``restart(N.AVG)`` adopts.  Float32 / float64 engines
        on one GPU without graph replay (``PdlpError`` otherwise)."""
        N.check(self.lib.pdlp_halpern_iterate(self.h, int(iters)), "pdlp_halpern_iterate")

    def halpern_fixed_point(self) -> Tuple[float, float, float]:
        """``(||dx||^2, dx'K'dy, ||dy||^2)`` of the last Halpern iteration (``pdlp_halpern_fixed_point``, include/pdlp_hip.h):
        ``dx, dy`` = the iterate before that iteration (``N.PREV``) minus its candidate (``N.AVG``).  One vector pass and one product;
        ``rules.fixed_point_error`` forms the residual from them.  Synchronises (it reads the three sums)."""
        N.check(self.lib.pdlp_halpern_fixed_point(self.h), "pdlp_halpern_fixed_point")
        out = (C.c_double * N.NRED)()
        N.check(self.lib.pdlp_read_red(self.h, out), "pdlp_read_red")
        return out[0], out[1], out[2]

    def adaptive_retry(self):
        """discard the adaptive iteration just taken (its trial was rejected: ``scalars()["accepted"] == 0``) so that it can be
        issued again with the shrunk step size -- ``pdlp_adaptive_retry`` (include/pdlp_hip.h), SURVEY quirk Q1's optional flag"""
        N.check(self.lib.pdlp_adaptive_retry(self.h), "pdlp_adaptive_retry")
        # the next dual half-step recomputes K x from the WHOLE restored x; sharded iterations exchange xbar and y only, so the other
        # ranks' blocks of that buffer are not current: gather them (over the process group, whichever driver runs the iterations)
        self._gather(N.BUF_X_CUR)

    # ---- restart machinery --------------------------------------------------------------------------
    def flush_average(self, adaptive: bool = True):
        """close the averaging period before a restart check (after ``kkt(CUR)``: include/pdlp_hip.h, pdlp_flush_average)"""
        N.check(self.lib.pdlp_flush_average(self.h, int(bool(adaptive))), "pdlp_flush_average")

    def compute_average(self):
        N.check(self.lib.pdlp_compute_average(self.h), "pdlp_compute_average")

    def _residuals(self, omega: float) -> dict:
        """the sums of ``pdlp_kkt_local`` / ``pdlp_report_local`` over all ranks -> residuals, gap and KKT error (helpers.py:53-108)"""
        self._reduce_sums()
        out = (C.c_double * 6)()
        N.check(self.lib.pdlp_kkt_finish(self.h, float(omega), out), "pdlp_kkt_finish")
        self._peer_check()                       # (the stream has been synchronised: a wait that gave up shows now)
        return dict(pr=out[0], dr=out[1], gap=out[2], p=out[3], d_adj=out[4], kkt=out[5])

    def kkt(self, which: int, omega: float, unscaled: bool = False) -> dict:
        """compute_residuals_and_duality_gap + KKT_error at CUR / AVG / PREV (helpers.py:53-108)."""
        if self.exact is not None or self.comm is not None:      # (one GPU, the handle's own matrix: pdlp_kkt_local refreshes them)
            self._ensure_anchors()
        if self.delta:
            # the current iterate is evaluated from the anchors (its pending dy was gathered by the iteration); a candidate
            # from the float32 difference candidate - current, which every rank forms in full
            if which != N.CUR:
                self._gather_iterate(N.CUR)
                self._gather_iterate(which)
        else:
            self._gather_iterate(which)
        N.check(self.lib.pdlp_kkt_local(self.h, which, int(unscaled)), "pdlp_kkt_local")
        return self._residuals(omega)

    def report(self, which: int = N.CUR, unscaled: bool = False, omega: float = 1.0) -> dict:
        """The solution report of an iterate (``pdlp_report_local``, include/pdlp_hip.h): ``y``, ``reduced_costs`` =
        project_lambda_box(c - K'y) and ``row_activity`` = K x (this rank's blocks when sharded; of the un-preconditioned problem
        with ``unscaled``: y_u = D_row y, lam_u = lam / D_col, (K x)_u = (K x) / D_row), and the residual dict of ``kkt``
        (helpers.py:53-108).  The products are always multiplied out (never the carried or running ones) and the solver's state is
        left as it is: a report taken between two ``iterate`` calls changes no later bit."""
        if self.exact is not None:
            # the handle's matrix is the float32 rounding of the true one: the report comes from the true matrix (the float64
            # engine behind the anchors, which holds no state of the solve)
            x, y = self.get_iterate(which)
            self.exact.set_iterate(x, y)
            return self.exact.report(N.CUR, unscaled, omega)
        self._gather_iterate(which)
        rc = torch.empty(self.nl, dtype=self.dtype, device=self.device)
        act = torch.empty(self.ml, dtype=self.dtype, device=self.device)
        N.check(self.lib.pdlp_report_local(self.h, int(which), int(bool(unscaled)), rc.data_ptr(), act.data_ptr()), "pdlp_report_local")
        res = self._residuals(omega)
        _, y = self.get_iterate(which)
        if unscaled:
            y = y * self.d_row
        return dict(y=y, reduced_costs=rc, row_activity=act, **res)

    def restart(self, which: int):
        N.check(self.lib.pdlp_restart(self.h, which), "pdlp_restart")

    def restart_distance(self) -> Tuple[float, float]:
        """(||x - x_last_restart||^2, ||y - y_last_restart||^2) over all ranks (enhancements.py:74-75)"""
        N.check(self.lib.pdlp_restart_distance_local(self.h), "pdlp_restart_distance_local")
        self._reduce_sums()
        out = (C.c_double * N.NRED)()
        N.check(self.lib.pdlp_read_red(self.h, out), "pdlp_read_red")
        return out[0], out[1]

    def mark_restart_point(self):
        N.check(self.lib.pdlp_mark_restart_point(self.h), "pdlp_mark_restart_point")

    # ---- infeasibility detection (opt-in) ---------------------------------------------------------------
    INFEAS_STATUS = (None, "DUAL_INFEASIBLE", "PRIMAL_INFEASIBLE")          # enhancements.py:142,159,161

    def infeas_reset(self):
        """lam_prev = 0 (pdhg.py:39-40)"""
        N.check(self.lib.pdlp_infeas_reset(self.h), "pdlp_infeas_reset")

    def detect_infeasibility(self, tol: float, diagnostics: bool = False):
        """detect_infeasibility (enhancements.py:80-161) for the step just taken, including the lambda of
        pdhg.py:90 and the lam_prev update of pdhg.py:101.  Returns the reference's status string or None."""
        N.check(self.lib.pdlp_infeas_begin(self.h), "pdlp_infeas_begin")
        if self.comm is not None:
            self.comm.all_gather(self.buffer(N.BUF_DX))
            self.comm.all_gather(self.buffer(N.BUF_DY))
            if self.delta:      # lambda = proj(c - K'y) multiplies the COMPLETE y; delta iterations exchange only the differences
                self._gather(N.BUF_Y_CUR)
        N.check(self.lib.pdlp_infeas_local(self.h, float(tol)), "pdlp_infeas_local")
        self._reduce_sums()
        st, diag = C.c_int32(0), (C.c_double * 8)()
        N.check(self.lib.pdlp_infeas_finish(self.h, float(tol), C.byref(st), diag), "pdlp_infeas_finish")
        status = self.INFEAS_STATUS[st.value]
        return (status, list(diag)) if diagnostics else status

    # ---- populations of points (fishnet) ------------------------------------------------------------------
    MV_WIDTHS = (8, 16, 32)

    def mv_steps(self, X: torch.Tensor, Y: torch.Tensor, steps: int, eta: float, omega: float, theta: float = 1.0):
        """``steps`` fixed-step PDHG iterations on every column of X (n x j) / Y (m x j), in place -- PDHG_step
        (spectral_casting.py:254-293); j in MV_WIDTHS, one pass over each matrix per step for all j points."""
        j = self._mv_check(X, Y)
        work = self._mv_work.get(j)         # kept per width: stream-ordered reuse, no allocation or sync per call
        if work is None:
            work = self._mv_work[j] = torch.empty((2 * self.n + self.m) * j, dtype=self.dtype, device=self.device)
        N.check(self.lib.pdlp_mv_steps(self.h, j, int(steps), float(eta), float(omega), float(theta), X.data_ptr(), Y.data_ptr(),
                                       work.data_ptr()), "pdlp_mv_steps")

    def mv_gap(self, X: torch.Tensor, Y: torch.Tensor) -> list:
        """signed duality gap (adjusted dual - primal objective) of every column -- get_best_pts (spectral_casting.py:215-234)"""
        j = self._mv_check(X, Y)
        work = torch.empty(256 * j * 4 + j * 4, dtype=torch.float64, device=self.device)
        out = (C.c_double * j)()
        N.check(self.lib.pdlp_mv_gap(self.h, j, X.data_ptr(), Y.data_ptr(), work.data_ptr(), out), "pdlp_mv_gap")
        return list(out)

    def mv_product(self, X: torch.Tensor) -> torch.Tensor:
        """K X for a population X (n x j, j in MV_WIDTHS) in one pass over K -- ``pts_y = K @ pts`` (spectral_casting.py:100)"""
        Y = torch.empty(self.m, int(X.shape[1]) if X.dim() == 2 else 0, dtype=self.dtype, device=self.device)
        j = self._mv_check(X, Y)
        N.check(self.lib.pdlp_mv_product(self.h, j, X.data_ptr(), Y.data_ptr()), "pdlp_mv_product")
        return Y

    def mv_combine(self, V: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
        """V @ W for a population V (rows x j, j <= 32) and weights W (j x nw, nw <= 32) -- the convex combinations of the breeding
        rounds (spectral_casting.py:133-141)"""
        V, W = V.contiguous(), W.to(device=self.device, dtype=self.dtype).contiguous()
        rows, j = V.shape
        nw = int(W.shape[1])
        if W.shape[0] != j or not (1 <= j <= 32 and 1 <= nw <= 32) or V.dtype != self.dtype or V.device != self.device:
            raise ValueError(f"mv_combine: {tuple(V.shape)} @ {tuple(W.shape)}")
        out = torch.empty(rows, nw, dtype=self.dtype, device=self.device)
        N.check(self.lib.pdlp_mv_combine(N.PDLP_F32 if self.dtype == torch.float32 else N.PDLP_F64, rows, j, V.data_ptr(), W.data_ptr(), nw,
                                         out.data_ptr(), self.stream.cuda_stream), "pdlp_mv_combine")
        return out

    def _mv_check(self, X, Y) -> int:
        if self.comm is not None:
            raise N.PdlpError("the population kernels run on one GPU")
        j = int(X.shape[1]) if X.dim() == 2 else 0          # (anything but a matrix: refused below like every other shape)
        ok = (X.dim() == 2 and Y.dim() == 2 and X.shape == (self.n, j) and Y.shape == (self.m, j) and j in self.MV_WIDTHS
              and X.is_contiguous() and Y.is_contiguous() and X.dtype == self.dtype == Y.dtype and X.device == self.device == Y.device)
        if not ok:
            raise ValueError(f"population of {tuple(X.shape)} / {tuple(Y.shape)}: need contiguous n x j and m x j, j in {self.MV_WIDTHS}")
        return j

    # ---- products -----------------------------------------------------------------------------------
    def spmv(self, v_full: torch.Tensor, transpose: bool = False) -> torch.Tensor:
        """K v (or K' v) for this rank's rows; ``v_full`` must be complete."""
        v = as_vec(v_full, self.m if transpose else self.n, self.device, self.dtype)
        out = torch.empty(self.nl if transpose else self.ml, dtype=self.dtype, device=self.device)
        N.check(self.lib.pdlp_spmv(self.h, int(transpose), v.data_ptr(), out.data_ptr()), "pdlp_spmv")
        return out

    def power_iteration(self, b0: torch.Tensor, iters: int = 100) -> float:
        """spectral_norm_estimate_torch (helpers.py:41-51) with the start vector given."""
        b0 = as_vec(b0, self.n, self.device, self.dtype)
        if self.comm is None:
            wn = torch.empty(self.n, dtype=self.dtype, device=self.device)
            wm = torch.empty(self.m, dtype=self.dtype, device=self.device)
            s = C.c_double(0)
            N.check(self.lib.pdlp_power_iteration(self.h, b0.data_ptr(), int(iters), wn.data_ptr(), wm.data_ptr(), C.byref(s)),
                    "pdlp_power_iteration")
            return s.value
        # sharded: the same recurrence with the exchange between the two products (setup, runs once)
        b = b0.clone()
        t = torch.zeros(self.m, dtype=self.dtype, device=self.device)
        r0, r1 = self.rows
        c0, c1 = self.cols
        for _ in range(int(iters)):
            t[r0:r1] = self.spmv(b, False)
            self.comm.all_gather(t)
            b[c0:c1] = self.spmv(t, True)
            self.comm.all_gather(b)
            b /= torch.linalg.norm(b)
        t[r0:r1] = self.spmv(b, False)
        self.comm.all_gather(t)
        return float(torch.linalg.norm(t))

    def synchronize(self):
        self.stream.synchronize()
