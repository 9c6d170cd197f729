"""What exists only for sharded engines.  Three drivers of the iterations -- the ``torch.distributed`` loop (``_iterate_loop``), the
library's RCCL exchange (``enable_library_comm``), the direct exchange over HIP IPC (``enable_peer_exchange``); ``PdlpEngine.iterate``
picks -- the chunked exchange's plan, the cross-check that guards the two library drivers, the chunk tuner.  Mixed into ``PdlpEngine``."""
from __future__ import annotations

import ctypes as C
import sys
import time
from typing import Optional

import torch

from . import _native as N
from .comm import Comm


class Exchange:
    """the part of ``PdlpEngine`` that moves vectors between the ranks"""

    PEER_FORMS = ("whole product after the wait", "own-block panels between signal and wait", "push beside the own-block panels")

    # ---- the chunked exchange: plan and pieces -------------------------------------------------------------------------------
    def set_producer_pieces(self, on: bool):
        """results of split products leave piece by piece with a chunked exchange (default) or only when the half-step has finished
        (round-4 behaviour; A/B timing and tests).  Every rank must choose the same."""
        self.set_option(N.OPT_PRODUCER_PIECES, int(bool(on)))
        self.producer_pieces = bool(on)

    def set_exchange_chunks(self, chunks: int):
        """Sharded, tiled products: move the gathered vector in ``chunks`` pieces (piece c = a slice of EVERY rank's block) and
        multiply the panels a piece completes while the next piece is on the wire (include/pdlp_hip.h, pdlp_set_exchange_chunks).
        1 = one all-gather per product.  Every rank must choose the same number."""
        N.check(self.lib.pdlp_set_exchange_chunks(self.h, int(chunks)), "pdlp_set_exchange_chunks")
        self.xchunks = int(chunks)
        self._plans = {}

    def exchange_plan(self, transpose: int) -> list:
        """[(lo, hi), ...]: the element ranges (inside one rank's block) of the pieces in which the input of K xbar (0) / K'y (1) travels"""
        plan = self._plans.get(int(transpose))
        if plan is None:
            nc, b = C.c_int32(0), (C.c_int64 * 5)()
            N.check(self.lib.pdlp_exchange_plan(self.h, int(transpose), C.byref(nc), b), "pdlp_exchange_plan")
            plan = self._plans[int(transpose)] = [(int(b[c]), int(b[c + 1])) for c in range(nc.value)]
        return plan

    def split_info(self, transpose: int) -> dict:
        """how a sharded product is split so that its local panels overlap the all-gather (zeros: not split)"""
        out = (C.c_int32 * 4)()
        N.check(self.lib.pdlp_split_info(self.h, int(transpose), out), "pdlp_split_info")
        return dict(local_panels=(out[0], out[1]), local_groups=out[2], other_groups=out[3])

    def _half_in_pieces(self, dual: bool, a: int, full: torch.Tensor):
        """One half-step.  If the exchange that follows it is chunked its result leaves in the pieces of that plan: the rows of
        piece c (``pdlp_*_half_piece``), then piece c's all-gather -- issued behind those rows, it runs while piece c + 1's rows
        are multiplied.  Returns the pieces' handles, or None when the half-step went out whole (the caller exchanges afterwards).
        Every rank takes the same branch: the plan is a function of the block length and the piece count alone."""
        plan = self.exchange_plan(1 if dual else 0)        # the plan of the exchange that FOLLOWS: y after the dual, xbar after the primal
        lib, h = self.lib, self.h
        if len(plan) == 1 or not self.producer_pieces:
            N.check((lib.pdlp_dual_half if dual else lib.pdlp_primal_half)(h, a), "pdlp_dual_half" if dual else "pdlp_primal_half")
            return None
        piece = lib.pdlp_dual_half_piece if dual else lib.pdlp_primal_half_piece
        works = []
        for c, (lo, hi) in enumerate(plan):
            N.check(piece(h, a, c, len(plan)), "pdlp_dual_half_piece" if dual else "pdlp_primal_half_piece")
            works.append(self.comm.all_gather_piece(full, lo, hi))
        return works

    def _start_exchange(self, transpose: int, full: torch.Tensor, works):
        """issue the exchange of ``full`` now, asynchronously, unless its pieces are on their way already; returns the handles
        (a one-element list for a one-piece plan)"""
        if works is not None:
            return works
        plan = self.exchange_plan(transpose)
        if len(plan) == 1:
            return [self.comm.all_gather_async(full)]
        return [self.comm.all_gather_piece(full, lo, hi) for lo, hi in plan]

    def _exchange(self, transpose: int, full: torch.Tensor, works):
        """the input of the next product to every rank, in the pieces of its plan; the panels a piece completes are multiplied as
        soon as it is there (all but the last piece's: those belong to the half-step that follows)"""
        for c, w in enumerate(works):          # (one handle per piece of the plan, None = already there: _start_exchange is the only producer)
            if w is not None:
                w.wait()
            if c + 1 < len(works):
                N.check(self.lib.pdlp_half_chunk(self.h, int(transpose), c), "pdlp_half_chunk")

    # ---- driver 1: the torch.distributed loop ----------------------------------------------------------------------------------
    def _iterate_loop(self, iters: int, adaptive: bool):
        """``iters`` iterations as six ctypes calls and three torch collectives each; ``iterate`` has made delta mode's anchors valid"""
        a = int(adaptive)
        lib, h, comm = self.lib, self.h, self.comm
        # what the other ranks need of a half-step's result: xbar and y -- or, in delta mode, the float32 differences
        # x+ - x and y+ - y (half the bytes on the wire); all four live at fixed addresses
        red = self.buffer(N.BUF_RED)
        xbar = self.buffer(N.BUF_GDX if self.delta else N.BUF_XBAR)
        gdy = self.buffer(N.BUF_GDY) if self.delta else None
        for it in range(iters):
            # With a chunked exchange the result of a half-step leaves piece by piece (_half_in_pieces): piece c's all-gather is
            # issued behind the rows it is made of and runs while the rows of piece c + 1 are still being multiplied.
            wx = self._half_in_pieces(False, a, xbar)
            # the panels of K that meet this rank's own block of xbar are multiplied while the other blocks are still on the wire
            # (the exchange is issued first, asynchronously, so the panels go onto the handle's own stream: no fork / join); the
            # same for K' and y below
            wx = self._start_exchange(0, xbar, wx)
            N.check(lib.pdlp_dual_half_begin(h, a), "pdlp_dual_half_begin")
            self._exchange(0, xbar, wx)                    # K xbar needs every rank's block of xbar
            ynew = gdy if self.delta else self.buffer(N.BUF_Y_PREV)     # where the dual half-step writes (the buffers alternate)
            wy = self._half_in_pieces(True, a, ynew)
            ar = None
            if adaptive:
                # the rank's three sums of the step-size rule need only this iteration's partial sums: the kernel that adds them up
                # runs while y is on the wire.  With pieces their all-reduce queues up behind the pieces and is reduced while the
                # panels those pieces complete are multiplied (same sums: only the order in which independent work is issued differs)
                N.check(lib.pdlp_adaptive_reduce(h), "pdlp_adaptive_reduce")
                if wy is not None:
                    ar = comm.all_reduce_sum_async(red)
            wy_sent = wy is not None
            wy = self._start_exchange(1, ynew, wy)
            if it + 1 < iters:                             # (the new y is final: a rejected adaptive step is kept, quirk Q1)
                N.check(lib.pdlp_primal_half_begin(h), "pdlp_primal_half_begin")
            self._exchange(1, ynew, wy)                    # (no product under way after the last iteration: the pieces just arrive)
            if adaptive:
                if not wy_sent:
                    comm.all_reduce_sum(red)
                elif ar is not None:
                    ar.wait()
                N.check(lib.pdlp_adaptive_update(h), "pdlp_adaptive_update")
        if not adaptive and iters > 0:
            N.check(lib.pdlp_fixed_advance(h, iters), "pdlp_fixed_advance")

    # ---- the cross-check of a library driver against driver 1 --------------------------------------------------------------------
    def _cross_check(self, path_b: str, switch, cases, same, iters: int = 2, eta: float = 1e-2, trace=lambda what: None) -> bool:
        """``iters`` iterations from x = y = 0 through the torch.distributed loop (``switch(False)``) and through ``path_b``
        (``switch(True)``), once per entry of ``cases`` (adaptive?): does ``same(adaptive, (x, y, eta), (x, y, eta))`` hold every
        time on this rank?  Leaves the engine at x = y = 0, eta = 0 (a fresh handle's state) with ``path_b`` on."""
        zeros = lambda ln: torch.zeros(ln, dtype=self.dtype, device=self.device)
        ok = True
        for adaptive in cases:
            out = []
            for on in (False, True):
                switch(on)
                self.set_iterate(zeros(self.nl), zeros(self.ml))
                self.set_step(eta, 1.0, 1.0, 0)
                trace(f"cross-check: {'adaptive' if adaptive else 'fixed'}, {path_b if on else 'loop'}: state set")
                self.iterate(iters, adaptive)
                trace("  iterations issued")
                x, y = self.get_iterate(N.CUR)         # (synchronises)
                trace("  synchronised")
                self._peer_check()
                out.append((x, y, self.scalars()["eta"]))
            ok = same(adaptive, *out) and ok
        self.set_iterate(zeros(self.nl), zeros(self.ml))
        self.set_step(0.0, 1.0, 1.0, 0)
        return bool(ok)

    @staticmethod
    def _same_bits(a, b) -> bool:
        (x0, y0, e0), (x1, y1, e1) = a, b
        return bool(torch.equal(x0, x1) and torch.equal(y0, y1) and e0 == e1)

    def _cross_check_paths(self, iters: int = 2, eta: float = 1e-2) -> bool:
        """adaptive iterations through the library's own exchange: the loop's bits?  (the direct exchange stays out of it)"""
        saved_peer = self.peer_on
        if saved_peer:
            self.set_peer_exchange(False)
        same = lambda adaptive, a, b: self._same_bits(a, b) and bool(torch.isfinite(a[0]).all())
        ok = self._cross_check("library exchange", lambda on: setattr(self, "lib_comm", on), (True,), same, iters, eta)
        self.lib_comm = False                      # (the caller turns it on once every rank has agreed)
        if saved_peer:
            self.set_peer_exchange(True)
        return ok

    def _cross_check_peer(self, iters: int = 2, eta: float = 1e-2, trace=lambda what: None) -> bool:
        """fixed-step, then adaptive iterations through the direct exchange, in its ``local_first`` form: the loop's bits -- except
        that more than two ranks add the step-size rule's three sums in rank order here, in the collective's order there: 1e-5"""
        def same(adaptive, a, b):
            (x0, y0, e0), (x1, y1, e1) = a, b
            fin = bool(torch.isfinite(x1).all()) and bool(torch.isfinite(y1).all())
            if adaptive and self.comm.world > 2:
                close = lambda p, q: bool(((p - q).abs() <= 1e-5 * (1 + q.abs())).all())
                return fin and close(x1, x0) and close(y1, y0) and abs(e1 - e0) <= 1e-5 * abs(e0)
            return fin and self._same_bits(a, b)
        saved_lib, self.lib_comm = self.lib_comm, False
        self.set_peer_local_first(True)
        ok = self._cross_check("direct exchange", self.set_peer_exchange, (False, True), same, iters, eta, trace)
        self.lib_comm = saved_lib
        return ok

    # ---- driver 2: the exchange inside the library (RCCL) ----------------------------------------------------------------------
    @staticmethod
    def _loaded_rccl():
        """path of the RCCL library this process already has mapped (PyTorch's), so that the library joins the same one"""
        try:
            return next((line.split()[-1] for line in open("/proc/self/maps") if "librccl" in line), None)
        except OSError:
            return None

    def enable_library_comm(self, dist=None, group=None, rccl_path: Optional[str] = None, timeout: float = 120.0,
                            cross_check: bool = True) -> bool:
        """Give the handle its own RCCL communicator (``pdlp_comm_init``): ``iterate`` then is ONE library call per restart
        period -- half-steps, all-gathers and the step-size all-reduce enqueued back to back on the stream -- instead of six
        ctypes calls and three torch collectives per iteration.  Every step is agreed on by ALL ranks over the existing process
        group before the next one: (1) the library loads (``pdlp_comm_load``, rank local), (2) the id travels from rank 0,
        (3) ``pdlp_comm_init`` in a helper thread with ``timeout`` seconds -- a hang becomes a fallback --, (4) a round trip of
        both collectives against known values, (5) ``cross_check``: two adaptive iterations from one synthetic state through the
        torch.distributed loop and through the library path must agree bit for bit.  Any failure anywhere leaves all ranks on
        the torch.distributed loop.  Call before the iterate is set (the cross-check overwrites it and resets it to zero).
        ``rccl_path``: the library to dlopen (default: the librccl this process has mapped -- PyTorch's).  ``self.lib_comm_log``
        records what happened.  Returns whether the library path is on."""
        import threading
        if dist is None:
            if self.comm is None:
                return False
            comm = self.comm
        else:
            comm = Comm(group, dist)                             # (a group of one rank: the engine itself keeps no communicator)
        dist, group, rank, world = comm.dist, comm.group, comm.rank, comm.world
        agree = lambda ok: comm.agree(ok, self.device)           # (gloo = rehearsal on a shared card: flags through host tensors)
        log = self.lib_comm_log = []
        path = rccl_path if rccl_path is not None else self._loaded_rccl()
        cpath = None if path is None else path.encode()
        if not agree(self.lib.pdlp_comm_load(cpath) == 0):
            log.append("load failed on some rank")
            return False
        idbuf = (C.c_char * 128)()
        ok = 1
        if rank == 0 and self.lib.pdlp_comm_unique_id(cpath, idbuf) != 0:
            ok = 0
        t = torch.tensor(list(idbuf.raw) + [ok], dtype=torch.uint8, device=comm.coll_device(self.device))
        dist.broadcast(t, 0, group=group)
        raw = bytes(t.cpu().tolist())
        if not raw[128]:
            log.append("unique id failed")
            return False
        C.memmove(idbuf, raw[:128], 128)
        res = {}

        def init():
            res["rc"] = self.lib.pdlp_comm_init(self.h, cpath, idbuf, rank, world)
        th = threading.Thread(target=init, daemon=True)
        th.start()
        th.join(timeout)
        if th.is_alive():
            self._comm_init_thread = th          # poisoned: the handle is never destroyed while that thread lives (__del__)
        if not agree((not th.is_alive()) and res.get("rc") == 0):
            log.append(f"init failed or timed out (this rank: alive={th.is_alive()}, rc={res.get('rc')})"
                       + ("; the handle is poisoned (a thread is still inside pdlp_comm_init): end this process rather than reuse it" if th.is_alive() else ""))
            return False
        # round trip: all-gather of a full-length vector and the 8-double all-reduce (rank-local errors are caught, so that
        # every rank reaches the agreement below)
        ok = 1
        try:
            dx, red = self.buffer(N.BUF_DX), self.buffer(N.BUF_RED)
            dx.zero_()
            dx[self.cols[0]:self.cols[1]] = rank + 1
            red.fill_(rank + 1)
            N.check(self.lib.pdlp_comm_all_gather(self.h, N.BUF_DX), "pdlp_comm_all_gather")
            N.check(self.lib.pdlp_comm_all_reduce_red(self.h), "pdlp_comm_all_reduce_red")
            self.stream.synchronize()
            want = torch.arange(1, world + 1, device=self.device, dtype=dx.dtype).repeat_interleave(self.nl)
            ok = int(torch.equal(dx, want) and bool((red == world * (world + 1) / 2).all()))
            dx.zero_()
            red.zero_()
        except N.PdlpError:
            ok = 0
        if not agree(ok):
            log.append("round trip wrong")
            return False
        if cross_check:
            try:
                same = int(self._cross_check_paths())
            except N.PdlpError:
                same = 0
            if not agree(same):
                self.lib_comm = False
                log.append("cross-check against the torch.distributed loop differs")
                return False
            log.append("cross-check: 2 adaptive iterations bit-identical on both paths")
        self.lib_comm = True
        return True

    # ---- driver 3: the direct exchange (pdlp_peer_*), iterations without collectives ---------------------------------------------
    def enable_peer_exchange(self, cross_check: bool = True, timeout_ms: Optional[int] = None, local_first: bool = False) -> bool:
        """Connect the ranks' handles over HIP IPC (``pdlp_peer_export`` / ``pdlp_peer_connect``, include/pdlp_hip.h): ``iterate`` then
        is ONE library call per restart period with NO collective in it -- every half-step stores its block of the exchanged vector
        straight into the other ranks' memory (xGMI between the GPUs of a node) and a flag follows; the step-size rule's sums travel
        with the flag.  At most 8 ranks, all on one node.  Every step is agreed on by all ranks over the process group: export,
        connect, and (``cross_check``) two fixed-step iterations that must equal the torch.distributed loop bit for bit plus two
        adaptive ones that must agree to 1e-5 (the ranks' three sums are added in rank order here, in the collective's order there;
        identical for two ranks).  Any failure leaves all ranks where they were.  Call before the iterate is set (the cross-check
        overwrites it and resets it to zero).  ``self.peer_log`` records what happened.  Returns whether the direct exchange is on.
        ``local_first``: split products with the own block's panels between signal and wait (``PDLP_OPT_PEER_LOCAL_FIRST``; the
        cross-check always runs in that form -- it is the one whose partial sums are grouped like the loop's)."""
        if self.comm is None or not hasattr(self.comm, "dist"):
            return False
        comm = self.comm
        dist, group, rank, world = comm.dist, comm.group, comm.rank, comm.world
        agree = lambda ok: comm.agree(ok, self.device)
        cdev = comm.coll_device(self.device)
        log = self.peer_log = []
        t_start = time.time()

        def trace(what):                                         # (PDLP_PEER_TRACE=1: where a first multi-GPU run spends its time)
            if self.knobs.peer_trace:
                sys.stderr.write(f"[peer exchange, rank {rank}, {time.time() - t_start:7.2f} s] {what}\n")
                sys.stderr.flush()

        if not agree(2 <= world <= 8):
            log.append(f"{world} ranks: the direct exchange connects 2 to 8")
            return False
        nb = N.PEER_INFO_BYTES
        info = (C.c_char * nb)()
        rc = self.lib.pdlp_peer_export(self.h, info)
        trace(f"exported (rc {rc}); the workspace ({self.workspace.numel() >> 20} MB) lies in an allocation of "
              f"{int.from_bytes(info.raw[232:240], 'little') >> 20} MB")
        mine = torch.tensor(list(info.raw) + [int(rc == 0)], dtype=torch.uint8, device=cdev)
        every = torch.empty(world * (nb + 1), dtype=torch.uint8, device=cdev)
        dist.all_gather_into_tensor(every, mine, group=group)
        raw = bytes(every.cpu().tolist())
        if not all(raw[q * (nb + 1) + nb] for q in range(world)):
            log.append(f"export failed on some rank (this rank: rc={rc})")
            return False
        infos = b"".join(raw[q * (nb + 1):q * (nb + 1) + nb] for q in range(world))
        trace("infos gathered")
        # one rank at a time (a few milliseconds each): N processes mapping each other's memory at the same moment is a first on any
        # machine this runs on, and a rank that never returns from hipIpcOpenMemHandle is then easy to tell apart in PDLP_PEER_TRACE
        # (the hang that did occur -- allocations with bit 31 of their size set -- is kept out by pdlp_peer_export / exportable_bytes)
        rc = 0
        for r in range(world):
            if r == rank:
                rc = self.lib.pdlp_peer_connect(self.h, rank, world, infos, 0)
                trace(f"connected (rc {rc})")
            agree(1)
        if not agree(rc == 0):
            log.append(f"connect failed on some rank (this rank: rc={rc})")
            if rc == 0:
                self.lib.pdlp_peer_close(self.h)
            return False
        if timeout_ms is not None:
            self.set_option(N.OPT_PEER_TIMEOUT_MS, int(timeout_ms))
        self.peer_on = True
        self.set_option(N.OPT_PEER_EXCHANGE, 1)
        if cross_check:
            try:
                same = int(self._cross_check_peer(trace=trace))
            except N.PdlpError as e:
                log.append(f"cross-check raised: {e}")
                same = 0
            trace(f"cross-check done on this rank: {same}")
            if not agree(same):
                log.append("cross-check against the torch.distributed loop differs")
                self.disable_peer_exchange()
                return False
            log.append("cross-check: 2 fixed-step iterations bit-identical, 2 adaptive ones within 1e-5 of the torch.distributed loop")
        self.set_peer_local_first(local_first)
        return True

    def set_peer_local_first(self, on: bool):
        self.peer_local_first = bool(on)
        self.set_option(N.OPT_PEER_LOCAL_FIRST, int(bool(on)))

    def set_peer_push(self, on: bool):
        """``PDLP_OPT_PEER_PUSH``: the block leaves by a copy kernel on a side stream, beside the own block's panels of the next product
        (the form for 2 and 4 ranks, where those panels are long enough to hide the links)"""
        self.peer_push = bool(on)
        self.set_option(N.OPT_PEER_PUSH, int(bool(on)))

    def set_peer_form(self, form: int):
        """0: signal, wait, whole product; 1: own-block panels between signal and wait; 2: push kernel beside the own-block panels"""
        self.set_peer_local_first(form == 1)
        self.set_peer_push(form == 2)
        self.peer_form = int(form)

    def disable_peer_exchange(self):
        self.peer_on = False
        N.check(self.lib.pdlp_peer_close(self.h), "pdlp_peer_close")

    def set_peer_exchange(self, on: bool):
        """use (or not) a connected direct exchange for the iterations"""
        st = self.peer_status()
        self.peer_on = bool(on) and st["connected"]
        self.set_option(N.OPT_PEER_EXCHANGE, int(self.peer_on))

    def peer_status(self) -> dict:
        out = (C.c_int32 * 4)()
        N.check(self.lib.pdlp_peer_status(self.h, out), "pdlp_peer_status")
        return dict(connected=bool(out[0]), enabled=bool(out[1]), gave_up_on=(out[2] - 1 if out[2] else None), exchanges=out[3])

    def _peer_check(self):
        """a wait of the direct exchange that gave up leaves incomplete vectors behind: never compute on"""
        if self.peer_on:
            st = self.peer_status()
            if st["gave_up_on"] is not None:
                raise N.PdlpError(f"direct exchange: rank {st['gave_up_on']} did not signal within the timeout "
                                  f"(exchange {st['exchanges']}); the iterate of this rank is incomplete")

    # ---- how many pieces: timed on this machine ----------------------------------------------------------------------------------
    def tune_exchange_chunks(self, reps: int = 4) -> dict:
        """Choose the number of pieces from what THIS machine does: time the all-gather of one gathered vector and this rank's
        product with K (max over the ranks).  Measured with stand-ins on one GPU (profiles/r03_split_chunks.log): one piece wins
        while the all-gather takes less than about half a product (the extra launches and partial-sum slots of a chunked exchange
        cost more than the overlap gains), two pieces win beyond that (-7 % at 8 ranks with a 0.2 ms all-gather, -12 % at 4 ranks
        with 0.3 ms).  Collective: every rank calls it (whatever kernel its own shard uses); all end up with the same choice.
        Call it before the iterate is set or between restart periods: ``pdlp_set_exchange_chunks`` refuses while a product is pending."""
        out = dict(chunks=1, all_gather_ms=None, product_ms=None)
        if self.comm is None:
            return out
        # Every decision below is GLOBAL: a rank whose shard is not tiled or not split (CSR fallback, too many row blocks) must not
        # leave before the collectives the others are about to issue, and all ranks must end up with the same number of pieces.
        mine = int(self.tiles[0] is not None and self.split_info(0)["local_groups"] > 0)
        flag = torch.tensor([-float(mine)], dtype=torch.float64, device=self.device)
        self.comm.all_reduce_max(flag)                      # max of the negated flags = -(min of the flags)
        if float(flag[0]) != -1.0:
            return out
        live = self.buffer(N.BUF_GDX if self.delta else N.BUF_XBAR)
        full = torch.zeros_like(live)                       # a scratch vector of the exchange's size: the live buffer is not touched
        vin = torch.zeros(self.n, dtype=self.dtype, device=self.device)
        res = torch.empty(self.ml, dtype=self.dtype, device=self.device)
        self.comm.dist.barrier(group=self.comm.group)
        ag = self._timed(lambda: self.comm.all_gather(full), reps, sync=True)
        prod = self._timed(lambda: N.check(self.lib.pdlp_spmv(self.h, 0, vin.data_ptr(), res.data_ptr()), "pdlp_spmv"), reps, sync=True)
        t = torch.tensor([ag, prod], dtype=torch.float64, device=self.device)
        self.comm.all_reduce_max(t)
        ag, prod = float(t[0]), float(t[1])
        chunks = 2 if ag > 0.5 * prod else 1
        self.set_exchange_chunks(chunks)
        # too few panels for pieces on some matrix of some rank: everybody stays with one all-gather (the plan is a function of the
        # block length alone, so this test gives the same answer everywhere; the reduction makes that a guarantee, not a hope)
        ok = torch.tensor([-float(all(len(self.exchange_plan(tr)) == chunks for tr in (0, 1)))], dtype=torch.float64, device=self.device)
        self.comm.all_reduce_max(ok)
        if chunks > 1 and float(ok[0]) != -1.0:
            chunks = 1
            self.set_exchange_chunks(1)
        out.update(chunks=chunks, all_gather_ms=round(ag, 4), product_ms=round(prod, 4))
        return out
