"""Which kernel multiplies each matrix of an engine: the CSR kernel, the CSR kernel over column-sorted row blocks, or the
panel-tiled one (the formats themselves: ``tiled.py``).  Mixed into ``PdlpEngine`` (engine.py)."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _native as N
from . import tiled as _tiled

# ``wants_tiles`` (measured: 1M x 1M with 100 per row 3.3x faster tiled, 500k x 500k with 20 per row 1.35x; with 5 per row CSR is ahead)
TILED_MIN_NNZ = 1 << 20          # non-zeros of the matrix
TILED_MIN_COLS = 1 << 16         # entries of the gathered vector
TILED_MIN_PER_ROW = 10           # non-zeros per row on average (``auto`` only)
PACKED_ITEMS_DEFAULT = True      # float32 handles: 7-byte items for every tile set that qualifies (PDLP_PACKED_ITEMS unset)


def packed_items_mode(env=None) -> str:
    """``PDLP_PACKED_ITEMS``, read when tiles are attached (for A/B in one process, like ``PDLP_TILED``): "0" the 32-bit index words,
    "1" 7-byte items or an error, anything else (unset: "auto") ``PACKED_ITEMS_DEFAULT`` for every tile set that qualifies"""
    return (os.environ if env is None else env).get("PDLP_PACKED_ITEMS", "auto") or "auto"


def wants_tiles(mode: str, rows: int, cols: int, nnz: int) -> bool:
    """Is a matrix a candidate for the tiled kernel under ``PDLP_TILED=mode``?  From the shape alone, so a run (and every rank of
    a sharded one) always takes the same kernel and therefore the same summation order: ``0`` never, ``1`` whenever there are
    rows, ``auto`` from the three thresholds on, ``time`` (or anything else) from the two size thresholds on."""
    if mode == "0" or rows == 0 or (mode != "1" and (cols < TILED_MIN_COLS or nnz < TILED_MIN_NNZ)):
        return False
    return not (mode == "auto" and nnz < TILED_MIN_PER_ROW * rows)


class KernelChoice:
    """the part of ``PdlpEngine`` that attaches matrix copies to the handle"""

    def tile_limits(self) -> dict:
        """what ``pdlp_attach_tiles`` accepts on this handle (the row-sum scratch and the partial-sum slots are sized at creation)"""
        out = (C.c_int32 * 6)()
        N.check(self.lib.pdlp_tile_limits(self.h, out), "pdlp_tile_limits")
        return dict(max_groups=out[0], max_blocks=out[1], rpt_max=out[2], cap=out[3], nt=out[4])

    def _maybe_attach_tiles(self):
        """The kernel of K and of K' (switches: ``knobs_from_env`` in engine.py): a candidate of ``wants_tiles`` gets tiles unless
        it is clustered or has too many row blocks; ``PDLP_TILED=time`` times both kernels on this device and keeps the faster
        one (not reproducible run to run; tuning only).  ``self.kernels`` records the choice per matrix."""
        kn = self.knobs
        mode = kn.tiled if self._want_tiles else "0"
        self.kernels = ["csr", "csr"]
        if kn.sorted == "1" and self._want_tiles:            # tests / tuning: sorted row blocks for every matrix the CSR kernel keeps
            for transpose in (0, 1):
                self.attach_sorted(transpose)
        if mode == "0":
            return
        lim = self.tile_limits()
        for transpose, (rp, ci, va), rows, cols in ((0, self.K, self.ml, self.n), (1, self.KT, self.nl, self.m)):
            if not wants_tiles(mode, rows, cols, int(va.numel())):
                continue
            with N.trace_range("pdlp: tile build (K')" if transpose else "pdlp: tile build (K)", self.stream):
                t = _tiled.build_tiles(rp, ci, va, rows, cols, lw=kn.tile_lw, rpt=kn.tile_rpt, groups=kn.tile_groups,
                                       max_groups=lim["max_groups"], kernel_limits=(lim["rpt_max"], lim["cap"], lim["nt"]))
            if t is None or t.nblk > lim["max_blocks"]:
                # clustered (banded, block structured): the CSR kernel, with every row block's items sorted by column
                if t is None and kn.sorted != "0":
                    self.attach_sorted(transpose, force=False)        # (only if the blocks' columns do cluster)
                continue
            if mode != "time":
                self.attach_tiles(transpose, t)
                continue
            g = torch.Generator(device=self.device).manual_seed(1)
            vin = torch.randn(cols, dtype=self.dtype, device=self.device, generator=g)
            out = torch.empty(rows, dtype=self.dtype, device=self.device)
            t_csr = self._time_spmv(transpose, vin, out)
            self.attach_tiles(transpose, t)
            if self._time_spmv(transpose, vin, out) >= t_csr:
                self.attach_tiles(transpose, None)

    def _timed(self, fn, reps: int, sync: bool = False) -> float:
        """ms per call of ``fn`` on the handle's stream: a warm-up call (waited for with ``sync``), then ``reps`` between two events"""
        fn()
        if sync:
            self.stream.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(self.stream)
        for _ in range(reps):
            fn()
        b.record(self.stream)
        b.synchronize()
        return a.elapsed_time(b) / reps

    def _time_spmv(self, transpose: int, vin: torch.Tensor, out: torch.Tensor, reps: int = 3) -> float:
        return self._timed(lambda: N.check(self.lib.pdlp_spmv(self.h, int(transpose), vin.data_ptr(), out.data_ptr()), "pdlp_spmv"), reps)

    def schedule_info(self, transpose: int) -> torch.Tensor:
        """The CSR kernel's row blocks of K (``transpose`` 0) or K' as the handle holds them (``pdlp_schedule_info``): an int64 view of
        shape (blocks + 1, 2) into the workspace, (first row, first non-zero) of every block and (rows, non-zeros) as the end"""
        nb, bp = C.c_int32(0), C.c_void_p()
        N.check(self.lib.pdlp_schedule_info(self.h, int(transpose), C.byref(nb), C.byref(bp)), "pdlp_schedule_info")
        off = bp.value - self.workspace.data_ptr()
        return self.workspace[off:off + (nb.value + 1) * 16].view(torch.int64).view(-1, 2)

    def attach_sorted(self, transpose: int, on: bool = True, force: bool = True):
        """Column-sorted copy of every row block's items for the CSR kernel (``pdlp_attach_sorted``; the format and when it pays:
        ``tiled.sorted_row_blocks``): for matrices whose entries cluster (banded, block structured) a wave's gathers then touch a
        few cache lines instead of one per lane.  Same sums."""
        transpose = int(transpose)
        if not on:
            N.check(self.lib.pdlp_attach_sorted(self.h, transpose, None, None, None), "pdlp_attach_sorted")
            self._sorted[transpose] = None
            self.kernels[transpose] = "csr"
            return
        _, ci, va = self.KT if transpose else self.K
        if int(va.numel()) == 0:
            return
        blk = self.schedule_info(transpose)
        built = _tiled.sorted_row_blocks(blk[:, 1], ci, va, force)       # (column 1: first non-zero of every block, and the end)
        if built is None:
            return
        sidx, sval, cbase, n_sorted = built
        N.check(self.lib.pdlp_attach_sorted(self.h, transpose, sidx.data_ptr(), sval.data_ptr(), cbase.data_ptr()), "pdlp_attach_sorted")
        self._sorted[transpose] = (sidx, sval, cbase)              # keep the arrays alive
        self.kernels[transpose] = f"csr, sorted row blocks ({n_sorted} of {blk.shape[0] - 1})"

    def attach_tiles(self, transpose: int, t: Optional["_tiled.Tiles"]):
        if t is None:
            N.check(self.lib.pdlp_attach_tiles(self.h, int(transpose), None), "pdlp_attach_tiles")
            self._plans = {}
            self.tiles[int(transpose)] = None
            self.kernels[int(transpose)] = "csr"
            return
        rem = [0, 0] + [None] * 8
        if t.nrem:
            rows = self.nl if transpose else self.ml
            t._work = torch.empty(int(t.rem_sptr.numel()) - 1, dtype=torch.float64, device=self.device)
            t._extra = torch.zeros(rows, dtype=self.dtype, device=self.device)
            t._extra32 = torch.zeros(rows, dtype=torch.float32, device=self.device) if self.mixed else None
            rem = [int(t.rem_rows.numel()), int(t.rem_sptr.numel()) - 1, t.rem_rows.data_ptr(), t.rem_rptr.data_ptr(), t.rem_sptr.data_ptr(),
                   t.rem_col.data_ptr(), t.rem_val.data_ptr(), t._work.data_ptr(), t._extra.data_ptr(),
                   None if t._extra32 is None else t._extra32.data_ptr()]
        rel, base = t.abi_tile_ptr()          # (int32 offsets relative to each row block's first item + the 64-bit bases; kept alive on t)
        desc = N.PdlpTiles(t.lw, t.rpt, t.cap, t.nblk, t.npanel, t.groups, t.idx.data_ptr(), t.val.data_ptr(), rel.data_ptr(), base.data_ptr(),
                           t.cnt.data_ptr(), *rem)
        N.check(self.lib.pdlp_attach_tiles(self.h, int(transpose), C.byref(desc)), "pdlp_attach_tiles")
        self._plans = {}
        self.tiles[int(transpose)] = t       # keep the arrays alive
        packed = self._maybe_attach_packed_items(int(transpose), t)
        # (a float32 engine's tiles are read as 7-byte items unless the name says otherwise; the other precisions know 32-bit words only)
        self.kernels[int(transpose)] = ("tiled" if t.groups == 1 else f"tiled/{t.groups} groups") + (f" + remainder {t.nrem}" if t.nrem else "") + \
            (", 32-bit items" if self._packed_items_apply() and not packed else "")

    def _packed_items_apply(self) -> bool:
        """7-byte items exist for the float32 kernels only (mixed precision shares the float32 tile set and keeps its 32-bit words)"""
        return self.dtype == torch.float32 and not self.mixed

    def _maybe_attach_packed_items(self, transpose: int, t: "_tiled.Tiles") -> bool:
        """7-byte items (``tiled.pack_items24``: 24-bit index words next to the 32-bit ones, which stay for the other precisions) for the
        float32 kernels of this handle: ``PDLP_PACKED_ITEMS`` = 0 never, 1 always (an error if a run does not fit), else
        ``PACKED_ITEMS_DEFAULT``.  Whether a tile set qualifies depends on the matrix alone, like the choice between tiles and CSR:
        every run decides the same (and the results are the same bits either way).  Recorded in ``t.stats`` (``packed_items``,
        ``bytes_per_nnz``) and in ``self.kernels``: a float32 engine's tile set that stays on the 32-bit words is named
        "..., 32-bit items"."""
        mode = packed_items_mode()
        want = self._packed_items_apply() and (mode == "1" or (mode != "0" and PACKED_ITEMS_DEFAULT))
        packed = False
        if want and not _tiled.packed_items_shape_ok(t):
            if mode == "1":
                raise N.PdlpError(f"PDLP_PACKED_ITEMS=1: the tile set does not qualify (cap {t.cap}, lw {t.lw}, or a row block of 2^30 items)")
        elif want:
            idx24 = torch.empty(t.items // 4 * 3, dtype=torch.int32, device=self.device)
            run_base = torch.empty(2 * (t.items // _tiled.GROUP + _tiled.P24_TAIL), dtype=torch.int32, device=self.device)
            flag = torch.empty(1, dtype=torch.int32, device=self.device)
            torch.cuda.current_stream(self.device).synchronize()          # (t.idx may have been written on another stream)
            N.check(self.lib.pdlp_pack_tile_items(t.idx.data_ptr(), t.items, t.lw, idx24.data_ptr(), run_base.data_ptr(), flag.data_ptr(),
                                                  self.stream.cuda_stream), "pdlp_pack_tile_items")
            self.stream.synchronize()
            if int(flag.item()) == 0:
                N.check(self.lib.pdlp_attach_packed_items(self.h, transpose, idx24.data_ptr(), run_base.data_ptr()), "pdlp_attach_packed_items")
                t._idx24, t._run_base = idx24, run_base       # keep the arrays alive
                packed = True
            elif mode == "1":
                raise N.PdlpError("PDLP_PACKED_ITEMS=1: a run of 64 sorted items spans more than 1023 columns")
        if not packed:
            t._idx24 = t._run_base = None
        nnz = max(int(t.stats.get("tiled", t.items)), 1)
        extra = int(t._run_base.numel()) * 4 if packed else 0
        t.stats["packed_items"] = packed
        t.stats["bytes_per_nnz"] = (t.items * (7 if packed else 8) + extra + int(t.cnt.numel()) * 4) / nnz
        return packed
