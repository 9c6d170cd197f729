"""Every rank of a sharded solve in ONE process on one GPU, driven in lockstep at the library-call level, with the test playing the
exchange: the blocks are copied between the ranks' buffers (fixed addresses: ``pdlp_buffer_ptr``) where a real run issues its
collectives, so the test decides when a piece "arrives".  In the spirit of tests/handle_model.py and tests/host_lp.py: importing this
module needs no GPU; only ``World`` does.

The call order is that of ``Exchange._iterate_loop`` (torchpdlp_amd/engine_exchange.py), which include/pdlp_hip.h documents at
``pdlp_set_exchange_chunks`` and ``pdlp_*_half_piece``: the half-step (whole, or piece by piece in the plan of the exchange that
follows), ``pdlp_*_half_begin``, then for every piece c of the plan [piece c arrives] ``pdlp_half_chunk(c)`` (c < C-1), and after the
last piece the half-step that consumes the vector.

What this module restates from the header alone (no planner code is read or imitated):
  ``plan_bounds``        piece c of a block of B elements starts at c*B/C rounded down to 64; one piece when B < 64*C
  ``panel_ready_piece``  after which piece every column of a panel of the gathered vector is present on a rank
  ``piece_row_blocks``   the row blocks that hold the rows of an output piece (piece r starts at the first row block that begins at
                         or after its first element)

Delivery policies of ``World.iterate``:
  "upfront"  every piece is copied right after ``pdlp_*_half_begin``
  "staged"   at the start of every exchange the foreign part of every destination is filled with ``SENTINEL`` and piece c overwrites
             its ranges only when it "arrives": a panel multiplied before its last entry is there is off by 2^60
  eager=True (with "upfront") after the stage that MUST have consumed a set of panels -- ``pdlp_*_half_begin``: the local panels,
             ``pdlp_half_chunk(c)``: the panels piece c completes -- the device is synchronised and the sentinel is written over exactly
             those panels' columns; the values come back when the half-step has finished.  A library that defers panels to a later
             stage than the contract names reads the sentinel.
``SENTINEL`` is 2^60: finite (the kernel's weight-0 over-reads rely on 0 * finite = 0), a power of two, far from every value of the
iteration, and its sums stay inside float32.
"""
import ctypes as C

import numpy as np
import torch

SENTINEL = float(2 ** 60)
MAX_CHUNKS = 4


# ---------------------------------------------------------------------------------------------------------------------
# the header's contract, restated
# ---------------------------------------------------------------------------------------------------------------------
def plan_bounds(B, chunks):
    """[b_0 = 0, ..., b_C = B]: piece c = elements [b_c, b_c+1) of EVERY rank's block of B elements"""
    Cn = max(1, min(MAX_CHUNKS, int(chunks)))
    if B < 64 * Cn:
        Cn = 1
    return [(c * B // Cn) // 64 * 64 for c in range(Cn)] + [int(B)]


def panel_ready_piece(total, world, rank, lw, bounds):
    """For every panel (2^lw consecutive entries of a gathered vector of ``total`` = world * B entries, the last one ragged) on rank
    ``rank``: -1 when all its entries lie in the rank's own block (nothing to wait for), else the piece with which the last of its
    foreign entries arrives.  ``bounds``: ``plan_bounds`` of the block."""
    W, B = 1 << lw, total // world
    assert B * world == total and bounds[0] == 0 and bounds[-1] == B
    inner = np.asarray(bounds[1:-1], np.int64)
    out = []
    for p in range(-(-total // W)):
        c0, c1 = p * W, min((p + 1) * W, total)
        ready = -1
        for q in range(c0 // B, (c1 - 1) // B + 1):
            if q == rank:
                continue
            last = min(c1, (q + 1) * B) - 1 - q * B            # the highest offset of this panel inside block q
            ready = max(ready, int(np.searchsorted(inner, last, side="right")))
        out.append(ready)
    return out


def piece_row_blocks(rows_out, rows_per_block, bounds):
    """[rb_0, ..., rb_R]: output piece r of a product with ``rows_out`` rows is made of the row blocks [rb_r, rb_r+1)"""
    nblk = -(-rows_out // rows_per_block)
    return [min(nblk, -(-b // rows_per_block)) for b in bounds[:-1]] + [nblk]


def decision_margins(lp, seed, factor, omega, k0, iters, model=None):
    """the accept / reject decisions of ``iters`` adaptive steps of the float64 model and how far each was from the threshold:
    [(accepted, |eta - eta_bar| / eta_bar)]"""
    from tests import handle_model as hm
    m = model or hm.HandleModel(lp)
    m.set_iterate(*hm.start_point(lp, seed))
    m.set_step(factor * m.eta0, omega, 1.0, k0)
    out = []
    for _ in range(iters):
        eta = m.eta
        _, _, _, _, info = m.o.step_adaptive(m.x, m.y, m.eta, m.omega, m.theta, m.k + 1)
        out.append((bool(info["accepted"]), abs(eta - float(info["eta_bar"])) / float(info["eta_bar"])))
        m.iterate(1, True)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# a float64 numpy world: pins the padding and the permutation before a GPU is involved
# ---------------------------------------------------------------------------------------------------------------------
def csr_pair(lp, dtype, device):
    import torchpdlp_amd as tp
    t = lambda v, dt: torch.tensor(np.asarray(v), dtype=dt, device=device)
    return tp.CsrPair(lp.m, lp.n, t(lp.A.indptr, torch.int64), t(lp.A.indices, torch.int32), t(lp.A.data, dtype))


class NumpyWorld:
    """fixed-step PDHG over the blocks ``shard_arrays`` cuts, K applied block by block to the padded vectors, all in float64"""

    def __init__(self, lp, world):
        import scipy.sparse as sp
        from torchpdlp_amd.distributed import shard_arrays
        K = csr_pair(lp, torch.float64, "cpu")
        t = lambda v: torch.tensor(np.asarray(v), dtype=torch.float64)
        self.world, self.ranks = world, []
        for r in range(world):
            a = shard_arrays(K, t(lp.c), t(lp.q), t(lp.l), t(lp.u), lp.m_ineq, r, world, balance="rows")
            self.part = a["part"]
            mat = lambda rows, cols, csr: sp.csr_matrix((csr[2].numpy(), csr[1].numpy(), csr[0].numpy()), shape=(rows, cols))
            self.ranks.append(dict(K=mat(self.part.Bm, a["n"], a["K_rows"]), KT=mat(self.part.Bn, a["m"], a["KT_rows"]), rows=a["rows"], cols=a["cols"],
                                   n_ineq=a["m_ineq"] - a["rows"][0], **{k: a[k].numpy() for k in ("c", "q", "l", "u")}))

    def set_iterate(self, x, y):
        self.x = self.part.pad_cols(torch.tensor(x)).numpy().copy()
        self.y = self.part.pad_rows(torch.tensor(y)).numpy().copy()

    def iterate(self, iters, eta, omega, theta=1.0):
        for _ in range(iters):
            xn, xbar, yn = self.x.copy(), self.x.copy(), self.y.copy()
            for r in self.ranks:
                c0, c1 = r["cols"]
                xn[c0:c1] = np.clip(self.x[c0:c1] - (eta / omega) * (r["c"] - r["KT"] @ self.y), r["l"], r["u"])
                xbar[c0:c1] = xn[c0:c1] + theta * (xn[c0:c1] - self.x[c0:c1])
            for r in self.ranks:
                r0, r1 = r["rows"]
                yn[r0:r1] = self.y[r0:r1] + eta * omega * (r["q"] - r["K"] @ xbar)
                yn[r0:r0 + r["n_ineq"]] = np.maximum(yn[r0:r0 + r["n_ineq"]], 0.0)
            self.x, self.y = xn, yn

    def get_iterate(self):
        return self.part.unpad_cols(torch.tensor(self.x)).numpy(), self.part.unpad_rows(torch.tensor(self.y)).numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the world on the GPU
# ---------------------------------------------------------------------------------------------------------------------
class SilentComm:
    """rank ``rank`` of ``world`` whose collectives do nothing: the test moves the blocks itself"""
    backend, group = "fake", None

    def __init__(self, rank, world):
        self.rank, self.world = rank, world

    def all_gather(self, full):
        pass

    def all_reduce_sum(self, t):
        pass

    def all_gather_async(self, full):
        return None

    def all_gather_piece(self, full, lo, hi):
        return None

    def all_reduce_sum_async(self, t):
        return None


class World:
    """``world`` engines over the blocks of one HostLP (``shard_arrays(..., balance="rows")``), everything on the current stream.
    ``dtype``: of the matrix; ``engine_kw`` may hold ``vec_dtype`` / ``delta`` (mixed precision).  ``lw`` = None: the CSR kernel."""

    def __init__(self, lp, world, dtype, lw, rpt=1, **engine_kw):
        import torchpdlp_amd as tp
        from tests.host_lp import DEV
        from torchpdlp_amd import _native as N
        from torchpdlp_amd.distributed import shard_arrays
        from torchpdlp_amd.tiled import build_tiles
        assert 2 <= world <= 8
        self.N, self.lp, self.world, self.lw, self.rpt = N, lp, world, lw, rpt
        self.vec = engine_kw.get("vec_dtype") or dtype
        K = csr_pair(lp, dtype, DEV)
        t = lambda v: torch.tensor(np.asarray(v), dtype=self.vec, device=DEV)
        self.engs = []
        for r in range(world):
            args = shard_arrays(K, t(lp.c), t(lp.q), t(lp.l), t(lp.u), lp.m_ineq, r, world, vec_dtype=self.vec, balance="rows")
            self.part = args.pop("part")
            eng = tp.PdlpEngine(comm=SilentComm(r, world), **args, **engine_kw)
            for tr in (0, 1):
                eng.attach_tiles(tr, None)
                eng.attach_sorted(tr, on=False)
            if lw is not None:
                lim = eng.tile_limits()
                for tr, (rp, ci, va), rows, cols in ((0, eng.K, eng.ml, eng.n), (1, eng.KT, eng.nl, eng.m)):
                    tl = build_tiles(rp, ci, va, rows, cols, lw=lw, rpt=rpt, groups=1, max_groups=lim["max_groups"],
                                     kernel_limits=(lim["rpt_max"], lim["cap"], lim["nt"]))
                    assert tl is not None and tl.nrem == 0, (r, tr)
                    eng.attach_tiles(tr, tl)
                self.rows_per_block = lim["nt"] * rpt
            self.engs.append(eng)
        p = self.part
        self.Bn, self.Bm, self.np_, self.mp = p.Bn, p.Bm, p.np_, p.mp
        for r, e in enumerate(self.engs):
            assert e.cols == (r * p.Bn, (r + 1) * p.Bn) and e.rows == (r * p.Bm, (r + 1) * p.Bm) and (e.n, e.m) == (p.np_, p.mp)
        self._ready = {}
        self.kx_fresh = False              # K x of the current x is carried by the handles (pdlp_dual_half_begin is a no-op otherwise)
        self.chunks, self.producer_pieces, self.inline = 1, True, True
        self.configure(1, True, True)
        self.snapshots_checked = 0
        self.poisoned = {0: 0, 1: 0}       # entries the eager check has overwritten, per product

    # ---- switches that change at run time --------------------------------------------------------------------------------
    def configure(self, chunks, producer_pieces=True, inline=True):
        for e in self.engs:
            e.set_exchange_chunks(chunks)
            e.set_producer_pieces(producer_pieces)
            e.set_option(self.N.OPT_BEGIN_INLINE, int(inline))
        self.chunks, self.producer_pieces, self.inline = chunks, producer_pieces, inline

    def block(self, tr):
        """(block length, gathered length) of the input of K xbar (0) / K'y (1)"""
        return (self.Bm, self.mp) if tr else (self.Bn, self.np_)

    def plan(self, tr):
        """the pieces of the exchange of xbar (0) / y (1): the library's, the same on every rank, and the header's formula"""
        plans = [e.exchange_plan(tr) for e in self.engs]
        assert all(p == plans[0] for p in plans), plans
        b = plan_bounds(self.block(tr)[0], self.chunks)
        assert plans[0] == list(zip(b[:-1], b[1:])), (plans[0], b)
        return plans[0]

    def ready(self, tr, rank):
        key = (tr, rank, self.chunks)
        if key not in self._ready:
            B, total = self.block(tr)
            self._ready[key] = panel_ready_piece(total, self.world, rank, self.lw, plan_bounds(B, self.chunks))
        return self._ready[key]

    def is_split(self, tr, rank):
        return self.lw is not None and self.engs[rank].split_info(tr)["local_groups"] > 0

    # ---- state -----------------------------------------------------------------------------------------------------------
    def _t(self, v):
        from tests.host_lp import DEV
        return torch.tensor(np.asarray(v), dtype=self.vec, device=DEV)

    def set_iterate(self, x, y):
        xp, yp = self.part.pad_cols(self._t(x)), self.part.pad_rows(self._t(y))
        for e in self.engs:
            e.set_iterate(xp[e.cols[0]:e.cols[1]], yp[e.rows[0]:e.rows[1]])
        self.gather(self.N.BUF_X_CUR)
        self.gather(self.N.BUF_Y_CUR)
        self.kx_fresh = False

    def set_step(self, eta, omega, theta=1.0, k=0):
        for e in self.engs:
            e.set_step(eta, omega, theta, k)

    def own(self, e, full, tr):
        """rank e's own block of a gathered vector: x-like (tr = 0) or y-like (1)"""
        lo, hi = e.rows if tr else e.cols
        assert 0 <= lo < hi <= full.numel() and full.numel() == self.block(tr)[1]
        return full[lo:hi]

    def gathered(self, which):
        tr = int(which in (self.N.BUF_Y_CUR, self.N.BUF_Y_PREV, self.N.BUF_Y_AVG))
        return torch.cat([self.own(e, e.buffer(which), tr) for e in self.engs])

    def gather(self, which):
        """what an all-gather of buffer ``which`` leaves on every rank"""
        full = self.gathered(which)
        for e in self.engs:
            e.buffer(which).copy_(full)

    def get_iterate(self):
        x, y = self.gathered(self.N.BUF_X_CUR), self.gathered(self.N.BUF_Y_CUR)
        return self.part.unpad_cols(x).cpu().numpy().astype(np.float64), self.part.unpad_rows(y).cpu().numpy().astype(np.float64)

    def sums(self):
        x = torch.cat([e.buffer(self.N.BUF_X_SUM) for e in self.engs])
        y = torch.cat([e.buffer(self.N.BUF_Y_SUM) for e in self.engs])
        return self.part.unpad_cols(x).cpu().numpy().astype(np.float64), self.part.unpad_rows(y).cpu().numpy().astype(np.float64)

    def scalars(self):
        return [e.scalars() for e in self.engs]

    def state(self):
        """everything the bitwise checks compare: per rank the own blocks of x and y, the whole xbar, the sums' blocks, the scalar
        block and red"""
        N, out = self.N, []
        for e in self.engs:
            out.append(dict(x=self.own(e, e.buffer(N.BUF_X_CUR), 0).clone(), y=e.buffer(N.BUF_Y_CUR).clone(), xbar=e.buffer(N.BUF_XBAR).clone(),
                            x_sum=e.buffer(N.BUF_X_SUM).clone(), y_sum=e.buffer(N.BUF_Y_SUM).clone(),
                            scalars=e.buffer(N.BUF_SCALARS).clone(), red=e.buffer(N.BUF_RED).clone()))
        return out

    @staticmethod
    def same_bits(a, b):
        """the names of what differs between two ``state()``s"""
        return [f"rank {r}: {k}" for r, (sa, sb) in enumerate(zip(a, b)) for k in sa if not torch.equal(sa[k], sb[k])]

    # ---- one half-step, whole or in the pieces of the exchange that follows ---------------------------------------------------
    def _half(self, dual, a, by_piece):
        N = self.N
        tr_out = 1 if dual else 0                       # the exchange that follows moves y (1) after the dual, xbar (0) after the primal
        plan = self.plan(tr_out)
        outs = [e.buffer(N.BUF_Y_PREV if dual else N.BUF_XBAR) for e in self.engs]      # (where the half-step writes: fixed addresses)
        for e, out in zip(self.engs, outs):
            lib, h = e.lib, e.h
            if len(plan) == 1 or not self.producer_pieces or not by_piece:
                N.check((lib.pdlp_dual_half if dual else lib.pdlp_primal_half)(h, a), "half-step")
                continue
            blk, snaps = self.own(e, out, tr_out), []
            for c, (lo, hi) in enumerate(plan):
                N.check((lib.pdlp_dual_half_piece if dual else lib.pdlp_primal_half_piece)(h, a, c, len(plan)), "half-step piece")
                assert 0 <= lo < hi <= blk.numel()
                snaps.append(blk[lo:hi].clone())        # what piece c's collective would send
            for (lo, hi), s in zip(plan, snaps):
                assert torch.equal(s, blk[lo:hi]), f"rank {e.comm.rank}: output piece [{lo}, {hi}) of the {'dual' if dual else 'primal'} half-step changed after it was announced"
                self.snapshots_checked += 1
        if dual:
            self.kx_fresh = True
        if self._restore is not None:                   # (the eager check's sentinels: the values come back before anything else reads them)
            bufs, full = self._restore
            for b in bufs:
                b.copy_(full)
            self._restore = None
        return outs

    # ---- one exchange: begin, the pieces, the chunks ---------------------------------------------------------------------------
    def _poison(self, buf, tr, panels):
        W, total = 1 << self.lw, self.block(tr)[1]
        for p in panels:
            lo, hi = p * W, min((p + 1) * W, total)
            assert 0 <= lo < hi <= buf.numel() == total
            buf[lo:hi] = SENTINEL
            self.poisoned[tr] += hi - lo

    def _exchange(self, tr, bufs, a, policy, eager, begin=True):
        """``bufs``: every rank's full-length buffer of the vector that travels (own block just written)"""
        N, B = self.N, self.block(tr)[0]
        W = self.world
        plan = self.plan(tr)
        full = torch.cat([self.own(e, b, tr) for e, b in zip(self.engs, bufs)])
        if policy == "staged":
            for r, b in enumerate(bufs):
                v = b.view(W, B)
                v[:r] = SENTINEL
                v[r + 1:] = SENTINEL
        begun = []
        for r, e in enumerate(self.engs):
            if begin:
                N.check(e.lib.pdlp_primal_half_begin(e.h) if tr else e.lib.pdlp_dual_half_begin(e.h, a), "half_begin")
            # the local panels run now -- unless the product is not split on this rank, or (K) the K x cache has to be refreshed first
            begun.append(begin and self.is_split(tr, r) and (tr == 1 or self.kx_fresh))
        if eager and any(begun):
            torch.cuda.synchronize()                    # (the local panels may run on the library's side stream)
            for r, (e, b) in enumerate(zip(self.engs, bufs)):
                if begun[r]:
                    pa, pb = e.split_info(tr)["local_panels"]
                    ready = self.ready(tr, r)
                    assert [p for p, c in enumerate(ready) if c < 0] == list(range(pa, pb)), (r, pa, pb)
                    self._poison(b, tr, range(pa, pb))
            self._restore = (bufs, full)
        src = full.view(W, B)

        def deliver(c):
            lo, hi = plan[c]
            for r, b in enumerate(bufs):
                v = b.view(W, B)
                v[:r, lo:hi] = src[:r, lo:hi]
                v[r + 1:, lo:hi] = src[r + 1:, lo:hi]
        if policy == "upfront":
            for c in range(len(plan)):
                deliver(c)
        for c in range(len(plan)):
            if policy == "staged":
                deliver(c)
            if c + 1 < len(plan):
                for e in self.engs:
                    N.check(e.lib.pdlp_half_chunk(e.h, tr, c), "pdlp_half_chunk")
                if eager and any(begun):
                    torch.cuda.synchronize()
                    for r, b in enumerate(bufs):
                        if begun[r]:
                            self._poison(b, tr, [p for p, rc in enumerate(self.ready(tr, r)) if rc == c])

    # ---- iterations ------------------------------------------------------------------------------------------------------------
    _restore = None

    def iterate(self, iters, adaptive, policy="upfront", eager=False, by_piece=True):
        assert policy in ("upfront", "staged") and not (eager and policy != "upfront")
        N, a = self.N, int(adaptive)
        for it in range(iters):
            xbars = self._half(False, a, by_piece)
            self._exchange(0, xbars, a, policy, eager)
            ys = self._half(True, a, by_piece)
            if adaptive:
                for e in self.engs:
                    N.check(e.lib.pdlp_adaptive_reduce(e.h), "pdlp_adaptive_reduce")
                self.all_reduce(3)
            self._exchange(1, ys, a, policy, eager, begin=it + 1 < iters)
            if adaptive:
                for e in self.engs:
                    N.check(e.lib.pdlp_adaptive_update(e.h), "pdlp_adaptive_update")
        if not adaptive and iters > 0:
            for e in self.engs:
                N.check(e.lib.pdlp_fixed_advance(e.h, iters), "pdlp_fixed_advance")
        assert self._restore is None

    def all_reduce(self, count):
        """the test's own sum of red[0 .. count) over the ranks, in rank order, written back to every rank"""
        reds = [e.buffer(self.N.BUF_RED) for e in self.engs]
        tot = reds[0][:count].clone()
        for r in reds[1:]:
            tot += r[:count]
        for r in reds:
            r[:count] = tot

    def adaptive_retry(self, gather=True):
        for e in self.engs:
            self.N.check(e.lib.pdlp_adaptive_retry(e.h), "pdlp_adaptive_retry")
        self.kx_fresh = False
        if gather:                                       # x of the restored iterate must be complete before the next dual half-step
            self.gather(self.N.BUF_X_CUR)

    def kkt(self, omega):
        """a KKT pass at CUR: the gathers ``PdlpEngine.kkt`` does for an engine with a communicator, the summed red"""
        N = self.N
        self.gather(N.BUF_X_CUR)
        self.gather(N.BUF_Y_CUR)
        for e in self.engs:
            N.check(e.lib.pdlp_kkt_local(e.h, N.CUR, 0), "pdlp_kkt_local")
        self.all_reduce(6)
        outs = []
        for e in self.engs:
            out = (C.c_double * 6)()
            N.check(e.lib.pdlp_kkt_finish(e.h, float(omega), out), "pdlp_kkt_finish")
            outs.append(dict(zip(("pr", "dr", "gap", "p", "d_adj", "kkt"), out)))
        assert all(o == outs[0] for o in outs), outs
        return outs[0]

    def poison_foreign_x(self):
        """the foreign blocks of all three x buffers as a real sharded run leaves them: not current (here: unmistakably so)"""
        N = self.N
        for r, e in enumerate(self.engs):
            for which in (N.BUF_X_CUR, N.BUF_X_PREV, N.BUF_X_AVG):
                v = e.buffer(which)
                assert v.numel() == self.world * self.Bn
                v = v.view(self.world, self.Bn)
                v[:r] = SENTINEL
                v[r + 1:] = SENTINEL


# ---------------------------------------------------------------------------------------------------------------------
# the LP, the steps and the directed list of configurations (tests/test_shard_world_host.py checks on the CPU what the GPU tests
# assume of them; tests/test_gpu_shard_world.py runs them)
# ---------------------------------------------------------------------------------------------------------------------
LP_ARGS = (12800, 8041, 6, 31)       # sparse_lp: all four bound classes; m_ineq = 5120 falls inside rank 3's block of 8; every world
START_SEED = 3                       # pads n (8041 is prime), world 3 also pads m
STEP = dict(factor=1.0, omega=1.25, k0=0)                # fixed and adaptive runs: every decision of 13 steps at least 5 % clear
RETRY_STEP = dict(factor=50.0, omega=1.25, k0=100000)    # 50 x the safe step late in a solve: see test_retry_step_is_rejected
WORLDS, LWS = (2, 3, 4, 8), (6, 8, 11)
_lp = []


def world_lp():
    from tests.host_lp import sparse_lp
    if not _lp:
        _lp.append(sparse_lp(*LP_ARGS))
    return _lp[0]


# (world, lw, precision, chunks, options): "options" = also producer pieces off and PDLP_OPT_BEGIN_INLINE 0 against 1
CONFIGS = [
    (2, 6, "f32", 2, True), (2, 8, "f32", 3, False), (2, 11, "f32", 2, False), (2, 6, "f64", 4, False), (2, 11, "f64", 3, False),
    (3, 6, "f32", 3, False), (3, 8, "f32", 2, True), (3, 11, "f32", 4, False), (3, 8, "f64", 4, False), (3, 6, "f64", 2, False),
    (4, 6, "f32", 4, False), (4, 8, "f32", 2, False), (4, 11, "f32", 3, False), (4, 8, "f64", 3, True), (4, 11, "f64", 2, False),
    (4, 6, "f64", 1, False), (4, 8, "mixed", 2, False), (4, 6, "mixed", 3, False),
    (8, 6, "f32", 2, False), (8, 8, "f32", 4, True), (8, 8, "f32", 3, False), (8, 11, "f32", 2, False), (8, 6, "f32", 1, False),
    (8, 8, "f64", 4, False), (8, 6, "f64", 3, False), (8, 11, "f64", 4, False),
]


def config_properties(world, lw, chunks, rows_per_block=512):
    """what a configuration exercises, from the header's contract alone: per product (0: K over xbar, 1: K' over y) and rank the number
    of panels per stage ([local, piece 0, piece 1, ...]) and the row blocks of the output pieces, and the properties that follow"""
    lp = world_lp()
    Bn, Bm = -(-lp.n // world), -(-lp.m // world)
    W, out = 1 << lw, dict(stages={}, row_blocks={}, empty_phase=False, empty_piece=False, unsplit_rank=False, fully_split=True,
                           boundary_in_panel=False, ragged_panel=False)
    for tr, (B, rows_out) in enumerate(((Bn, Bm), (Bm, Bn))):
        bounds = plan_bounds(B, chunks)
        rb = piece_row_blocks(rows_out, rows_per_block, plan_bounds(rows_out, chunks))
        out["row_blocks"][tr] = rb
        out["boundary_in_panel"] |= B % W != 0
        out["ragged_panel"] |= (B * world) % W != 0
        counts = []
        for rank in range(world):
            ready = panel_ready_piece(B * world, world, rank, lw, bounds)
            counts.append([sum(1 for c in ready if c == s) for s in range(-1, len(bounds) - 1)])
        out["stages"][tr] = counts
        split = [c[0] > 0 and sum(c[1:]) > 0 for c in counts]
        out["fully_split"] &= all(split)
        out["unsplit_rank"] |= any(split) and not all(split)
        out["empty_phase"] |= any(s and len(c) > 2 and 0 in c[1:] for s, c in zip(split, counts))
        out["empty_piece"] |= any(split) and len(bounds) > 2 and any(a == b for a, b in zip(rb[:-1], rb[1:]))
    return out
