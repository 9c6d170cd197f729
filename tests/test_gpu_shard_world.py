"""Sharded iterations with every rank of the world in ONE process (tests/shard_world.py): the split products' plan (configure_split),
its launches (launch_mat, half_begin_t, half_chunk_t, half_piece) and the call order of ``Exchange._iterate_loop``, for worlds of 2, 3,
4 and 8 ranks, with the test playing the exchange -- so it can withhold a piece until its stage (policy "staged": what has not arrived is
2^60) and take a panel away after the stage that must have consumed it ("eager").

Bitwise (no tolerance: same plan, same grouping of the partial sums), fixed and adaptive steps, 3 iterations from a random start:
staged = upfront, eager = upfront, piece-by-piece half-steps = whole half-steps, every announced output piece = the final block,
producer pieces off = on, PDLP_OPT_BEGIN_INLINE 0 = 1 -- in x, y, xbar, the sums, the scalar block and red.

Against the float64 model of the UNSHARDED LP (tests/handle_model.py), with the tolerances and the scale rule of
tests/test_gpu_sequences.py: A_TOL for float64 and mixed worlds and B_TOL for float32 fixed-step worlds over 12 iterations; float32
adaptive worlds as tests/test_distributed.py holds them for two ranks (13 iterations: x within rtol 2e-4 + atol 2e-5, eta and the KKT
error within rtol 1e-4).  Adaptive runs take the model's accept / reject decisions: compared directly at iterations 1, 2, 3 and the
last (the scalar block shows the last iteration of a call), in between through k, eta_sum and eta.  Sharding only regroups sums, so none of these is loosened.  ``STATS`` keeps the largest deviation over its
tolerance per configuration (printed as SHARD-WORLD-STATS; PDLP_SHARD_WORLD_STATS=<file> writes it).

The adaptive retry on a sharded handle (pdlp_adaptive_retry's comment in include/pdlp_hip.h: x of the restored iterate must be complete
before the next half-step): worlds whose foreign x blocks are 2^60 when the retry comes, and ``PdlpEngine.adaptive_retry`` itself with a
communicator that records its calls.
"""
import ctypes as C
import gc
import json
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import handle_model as hm
from tests import shard_world as sw
from tests.host_lp import DEV
from tests.test_gpu_sequences import A_TOL, B_TOL
from torchpdlp_amd import _native as N

STATS = {}
_ONE = {}                            # the one world alive (at most 8 handles in the process)
_MODEL = {}
ENV = ("PDLP_RUNNING_KKT", "PDLP_NO_KTY_REUSE", "PDLP_GRAPH", "PDLP_DELTA", "PDLP_TILED", "PDLP_SORTED", "PDLP_BEGIN_INLINE",
       "PDLP_PRODUCER_PIECES", "PDLP_EXCHANGE_CHUNKS", "PDLP_LIB_COMM", "PDLP_TILE_LW", "PDLP_TILE_RPT", "PDLP_TILE_GROUPS")


@pytest.fixture(scope="module", autouse=True)
def _setup():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    N.load()
    t0 = time.time()
    yield
    _ONE.clear()
    gc.collect()
    summary = dict(wall_seconds=round(time.time() - t0, 2), worst=STATS)
    print("\nSHARD-WORLD-STATS " + json.dumps(summary))
    if os.environ.get("PDLP_SHARD_WORLD_STATS"):
        with open(os.environ["PDLP_SHARD_WORLD_STATS"], "w") as f:
            json.dump(summary, f, indent=1)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def model():
    if not _MODEL:
        _MODEL["m"] = hm.HandleModel(sw.world_lp())
    return _MODEL["m"]


def get_world(world, lw, prec):
    key = (world, lw, prec)
    if _ONE.get("key") != key:
        _ONE.clear()
        gc.collect()
        torch.cuda.synchronize()
        dtype = torch.float64 if prec == "f64" else torch.float32
        kw = dict(vec_dtype=torch.float64, delta=False) if prec == "mixed" else {}
        _ONE.update(key=key, world=sw.World(sw.world_lp(), world, dtype, lw, **kw))
    return _ONE["world"]


def start(w, step=sw.STEP):
    x, y = hm.start_point(sw.world_lp(), sw.START_SEED)
    w.set_iterate(x, y)
    w.set_step(step["factor"] * model().eta0, step["omega"], 1.0, step["k0"])
    for e in w.engs:                                     # (red is compared bit for bit: nothing of an earlier run in it)
        e.buffer(N.BUF_RED).zero_()
    return x, y


def model_run(adaptive, iters, checkpoints=()):
    """the float64 model's run from the common start, once per (mode, length): the same for every configuration"""
    key = (adaptive, iters, tuple(checkpoints))
    if key not in _MODEL:
        m = model()
        m.set_iterate(*hm.start_point(sw.world_lp(), sw.START_SEED))
        m.set_step(sw.STEP["factor"] * m.eta0, sw.STEP["omega"], 1.0, sw.STEP["k0"])
        accepted, done = [], 0
        for upto in list(checkpoints) + [iters]:
            m.iterate(upto - done, adaptive)
            done = upto
            accepted.append(bool(m.accepted))
        _MODEL[key] = dict(x=m.x.copy(), y=m.y.copy(), x_sum=m.x_sum.copy(), y_sum=m.y_sum.copy(), scalars=m.scalars(), accepted=accepted,
                           kkt=m.kkt(hm.CUR, sw.STEP["omega"]))
    return _MODEL[key]


def note(cfg, what, dev, bound):
    assert np.isfinite(dev), (cfg, what)
    s = STATS.setdefault("-".join(str(v) for v in cfg), dict(ratio=0.0))
    print(f"{cfg} {what}: deviation {dev:.3e}, bound {bound:.3e}, ratio {dev / bound:.3f}")
    if dev / bound > s["ratio"]:
        s.update(ratio=float(dev / bound), deviation=float(dev), bound=float(bound), what=what)
    return dev <= bound


# ---------------------------------------------------------------------------------------------------------------------
# the directed list
# ---------------------------------------------------------------------------------------------------------------------
def confirm_properties(w, cfg):
    """the cases a configuration was chosen for, from what the LIBRARY reports (split_info, exchange_plan, the tiles' panel and row
    block counts) beside the helper's function of the contract; that the list as a whole holds every case is asserted in
    tests/test_shard_world_host.py.  One case rests on the contract alone: the library does not report the row blocks of its output
    pieces, so ``empty_piece`` is the header's rule (``piece_row_blocks``) applied to the library's plan and row block count -- what
    the library then does with such a piece shows in the piece snapshots and in the comparison with whole half-steps."""
    world, lw, _, chunks, _ = cfg
    want = sw.config_properties(world, lw, chunks, w.rows_per_block)
    W = 1 << lw
    got = dict(empty_phase=False, empty_piece=False, unsplit_rank=False, fully_split=True, boundary_in_panel=False, ragged_panel=False)
    for tr in (0, 1):
        B, total = w.block(tr)
        plan = w.plan(tr)                                # (asserts: the same on every rank, and the header's formula)
        assert len(plan) == (chunks if B >= 64 * chunks else 1)
        rows_out = w.block(1 - tr)[0]
        rb = sw.piece_row_blocks(rows_out, w.rows_per_block, sw.plan_bounds(rows_out, chunks))
        got["boundary_in_panel"] |= B % W != 0
        got["ragged_panel"] |= total % W != 0
        split = []
        for r, e in enumerate(w.engs):
            assert e.tiles[tr] is not None and e.tiles[tr].npanel == -(-total // W) and e.tiles[tr].nblk == -(-rows_out // w.rows_per_block)
            info, ready = e.split_info(tr), w.ready(tr, r)
            local = [p for p, c in enumerate(ready) if c < 0]
            split.append(info["local_groups"] > 0)
            assert split[-1] == (len(local) > 0 and len(local) < len(ready)), (tr, r, info)
            if split[-1]:
                assert list(range(*info["local_panels"])) == local and info["other_groups"] > 0, (tr, r, info)
                counts = [sum(1 for c in ready if c == s) for s in range(len(plan))]
                got["empty_phase"] |= len(plan) > 1 and 0 in counts
            else:
                assert info == dict(local_panels=(0, 0), local_groups=0, other_groups=0)
        got["fully_split"] &= all(split)
        got["unsplit_rank"] |= any(split) and not all(split)
        got["empty_piece"] |= any(split) and len(plan) > 1 and any(a == b for a, b in zip(rb[:-1], rb[1:]))
    assert got == {k: want[k] for k in got}, (got, want)
    return got


def run(w, adaptive, iters=3, **kw):
    start(w)
    w.iterate(iters, adaptive, **kw)
    torch.cuda.synchronize()
    return w.state()


def check_bits(cfg):
    world, lw, prec, chunks, options = cfg
    w = get_world(world, lw, prec)
    w.configure(chunks, True, True)
    props = confirm_properties(w, cfg)
    for adaptive in (False, True):
        snaps, w.poisoned = w.snapshots_checked, {0: 0, 1: 0}
        ref = run(w, adaptive)
        assert all(bool(torch.isfinite(s[k]).all()) and float(s[k].abs().max()) < 1e6 for s in ref for k in ("x", "y", "xbar"))
        if chunks > 1:
            assert w.snapshots_checked >= snaps + 3 * 2 * world * 2        # every piece of every half-step of every rank
        assert w.same_bits(ref, run(w, adaptive, policy="staged")) == [], "staged delivery differs from upfront"
        assert w.same_bits(ref, run(w, adaptive, eager=True)) == [], "a panel was read after the stage that completes it"
        for tr in (0, 1):                                               # (the eager check did take panels away)
            assert (w.poisoned[tr] > 0) == any(w.is_split(tr, r) for r in range(world)), (tr, w.poisoned)
        assert w.same_bits(ref, run(w, adaptive, by_piece=False)) == [], "half-steps in pieces differ from whole half-steps"
        if options:
            w.configure(chunks, False, True)
            assert w.same_bits(ref, run(w, adaptive, policy="staged")) == [], "producer pieces off differs from on"
            w.configure(chunks, True, False)
            assert w.same_bits(ref, run(w, adaptive, policy="staged")) == [], "PDLP_OPT_BEGIN_INLINE 0 differs from 1"
            assert w.same_bits(ref, run(w, adaptive, eager=True)) == [], "begin on the side stream: a panel was read after its stage"
            w.configure(chunks, True, True)
    return props


def check_model(cfg):
    world, lw, prec, chunks, _ = cfg
    w = get_world(world, lw, prec)
    w.configure(chunks, True, True)
    ok = []
    for adaptive in (False, True):
        f32_adaptive = prec == "f32" and adaptive
        iters = 13 if f32_adaptive else 12
        # the first three adaptive iterations one call each, the rest in one (the products of K' are split inside a call only).  The
        # handle shows the decision of the LAST iteration of a call only, so iterations 1, 2, 3 and the last are compared with the
        # model's directly; the ones between through k, eta_sum and eta (each decision is at least 5 % clear in the model,
        # tests/test_shard_world_host.py: a different one moves eta by far more than the tolerance)
        checkpoints = (1, 2, 3) if adaptive else ()
        m = model_run(adaptive, iters, checkpoints)
        start(w)
        done = 0
        for upto, want in zip(list(checkpoints) + [iters], m["accepted"]):
            w.iterate(upto - done, adaptive, policy="staged")
            done = upto
            if adaptive:
                assert [bool(s["accepted"]) for s in w.scalars()] == [want] * world, (upto, want)
        x, y = w.get_iterate()
        sc, ref = w.scalars(), m["scalars"]
        assert all(s == sc[0] for s in sc) and sc[0]["k"] == ref["k"]
        got_kkt, ref_kkt = w.kkt(sw.STEP["omega"]), m["kkt"]
        tag = "adaptive" if adaptive else "fixed"
        if f32_adaptive:
            ok.append(note(cfg, f"{tag} x", float((np.abs(x - m["x"]) / (2e-5 + 2e-4 * np.abs(m["x"]))).max()), 1.0))
            ok.append(note(cfg, f"{tag} eta", abs(sc[0]["eta"] - ref["eta"]), 1e-4 * abs(ref["eta"])))
            ok.append(note(cfg, f"{tag} kkt", abs(got_kkt["kkt"] - ref_kkt["kkt"]), 1e-4 * abs(ref_kkt["kkt"])))
            continue
        tol = B_TOL if prec == "f32" else A_TOL
        xs, ys = w.sums()
        for what, g, r in (("x", x, m["x"]), ("y", y, m["y"]), ("x_sum", xs, m["x_sum"]), ("y_sum", ys, m["y_sum"])):
            ok.append(note(cfg, f"{tag} {what}", float(np.abs(g - r).max()), tol["iter"] * (1.0 + float(np.abs(r).max()))))
        for key in ("eta", "eta_sum", "w_pending"):
            ok.append(note(cfg, f"{tag} {key}", abs(sc[0][key] - ref[key]), tol["iter"] * (abs(ref[key]) if ref[key] else 1.0)))
        scale = 1.0 + abs(ref_kkt["p"]) + abs(ref_kkt["d_adj"])
        for key in ("pr", "dr", "gap", "p", "d_adj", "kkt"):
            ok.append(note(cfg, f"{tag} kkt:{key}", abs(got_kkt[key] - ref_kkt[key]), tol["kkt"] * scale))
    assert all(ok), STATS["-".join(str(v) for v in cfg)]


def pytest_generate_tests(metafunc):
    if "cfg" in metafunc.fixturenames:
        metafunc.parametrize("cfg,check", [(c, k) for c in sw.CONFIGS for k in ("bits", "model")],
                             ids=lambda v: v if isinstance(v, str) else "w{}-lw{}-{}-c{}{}".format(*v[:4], "-options" if v[4] else ""))


def test_world(cfg, check):
    (check_bits if check == "bits" else check_model)(cfg)


# ---------------------------------------------------------------------------------------------------------------------
# refused calls
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_calls():
    w = get_world(4, 8, "f64")
    w.configure(3, True, True)
    e = w.engs[1]
    lib, h = e.lib, e.h
    assert w.is_split(0, 1) and len(w.plan(0)) == 3
    start(w)
    # nothing pending: nothing is launched, whatever the chunk
    before = w.state()
    for c in (0, 1, 2, 3):
        assert lib.pdlp_half_chunk(h, 0, c) == 0 and lib.pdlp_half_chunk(h, 1, c) == 0
    assert lib.pdlp_half_chunk(h, 0, 4) == -1 and lib.pdlp_half_chunk(h, 0, -1) == -1
    torch.cuda.synchronize()
    assert w.same_bits(before, w.state()) == []
    for piece in (lib.pdlp_primal_half_piece, lib.pdlp_dual_half_piece):
        assert piece(h, 0, 3, 3) == -1 and piece(h, 0, 0, 5) == -1 and piece(h, 0, -1, 3) == -1 and piece(h, 0, 0, 0) == -1
    torch.cuda.synchronize()
    assert w.same_bits(before, w.state()) == []
    # a pending split product: chunks in order only; the last piece's chunk belongs to the half-step
    def second_iteration(poke):
        start(w)
        w.iterate(1, False)                              # (K x is carried from here on: pdlp_dual_half_begin runs the local panels)
        for r in w.engs:
            N.check(r.lib.pdlp_primal_half(r.h, 0))
        xbar = w.gathered(N.BUF_XBAR)
        for r in w.engs:
            r.buffer(N.BUF_XBAR).copy_(xbar)
            N.check(r.lib.pdlp_dual_half_begin(r.h, 0))
        if poke:
            assert lib.pdlp_half_chunk(h, 0, 1) == -3    # out of order
            assert lib.pdlp_half_chunk(h, 0, 0) == 0
            assert lib.pdlp_half_chunk(h, 0, 0) == -3    # twice
            assert lib.pdlp_half_chunk(h, 0, 1) == 0
            assert lib.pdlp_half_chunk(h, 0, 2) == 0     # the last piece: PDLP_OK, nothing launched
            assert lib.pdlp_half_chunk(h, 0, 3) == -3
            assert lib.pdlp_set_exchange_chunks(h, 2) == -3 and lib.pdlp_set_option(h, N.OPT_PRODUCER_PIECES, 0) == -3
        for r in w.engs:                                 # the half-step multiplies whatever no chunk call has
            N.check(r.lib.pdlp_dual_half(r.h, 0))
        torch.cuda.synchronize()
        return w.gathered(N.BUF_Y_CUR).clone()
    assert torch.equal(second_iteration(True), second_iteration(False))


# ---------------------------------------------------------------------------------------------------------------------
# the adaptive retry
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,lw", [(2, 8), (2, None), (8, 6), (8, None)], ids=lambda v: str(v))
def test_retry_restores_a_complete_x(world, lw):
    """a rejected trial (50 x the safe step, late in a solve: the first trial is accepted next to eta_bar, the second rejected --
    tests/test_shard_world_host.py), pdlp_adaptive_retry on every rank with the foreign blocks of all three x buffers at 2^60 (what a
    sharded run leaves there is not current either), the gather the header asks for, the iteration again: the model's, under A_TOL"""
    cfg = (world, lw, "f64", 2, "retry")
    w = get_world(world, lw, "f64")
    w.configure(2, True, True)
    m = model()
    x0, y0 = start(w, sw.RETRY_STEP)
    m.set_iterate(x0, y0)
    m.set_step(sw.RETRY_STEP["factor"] * m.eta0, sw.RETRY_STEP["omega"], 1.0, sw.RETRY_STEP["k0"])
    for want in (True, False):
        w.iterate(1, True, policy="staged")
        m.iterate(1, True)
        assert m.accepted == want and [bool(s["accepted"]) for s in w.scalars()] == [want] * world
    w.poison_foreign_x()
    w.adaptive_retry()
    m.adaptive_retry()
    ok = []

    def compare(tag):
        x, y = w.get_iterate()
        sc, ref = w.scalars(), m.scalars()
        assert all(s == sc[0] for s in sc) and sc[0]["k"] == ref["k"]
        for what, g, r in (("x", x, m.x), ("y", y, m.y)):
            ok.append(note(cfg, f"{tag} {what}", float(np.abs(g - r).max()), A_TOL["iter"] * (1.0 + float(np.abs(r).max()))))
        for key in ("eta", "eta_sum", "w_pending"):
            ok.append(note(cfg, f"{tag} {key}", abs(sc[0][key] - ref[key]), A_TOL["iter"] * (abs(ref[key]) if ref[key] else 1.0)))
    compare("after the retry")
    w.iterate(1, True, policy="staged")
    m.iterate(1, True)
    assert [bool(s["accepted"]) for s in w.scalars()] == [m.accepted] * world
    compare("the iteration again")
    got, ref = w.kkt(sw.RETRY_STEP["omega"]), m.kkt(hm.CUR, sw.RETRY_STEP["omega"])     # (K x carried from the refreshed product)
    scale = 1.0 + abs(ref["p"]) + abs(ref["d_adj"])
    for key in ("pr", "dr", "gap", "p", "d_adj", "kkt"):
        ok.append(note(cfg, f"kkt:{key}", abs(got[key] - ref[key]), A_TOL["kkt"] * scale))
    assert all(ok), STATS["-".join(str(v) for v in cfg)]


class RecordingComm(sw.SilentComm):
    """rank ``rank`` of ``world`` beside peers that never move: every gather fills the foreign blocks from the full vectors the test
    holds (by length: x-like or y-like), every call is recorded; the peers' share of the step-size rule's sums is what ``force`` says"""

    def __init__(self, rank, world, x_full, y_full):
        super().__init__(rank, world)
        self.full = {x_full.numel(): x_full, y_full.numel(): y_full}
        self.calls, self.force = [], None

    def _fill(self, name, full, lo=None, hi=None):
        self.calls.append((name, full.data_ptr()))
        src = self.full[full.numel()].to(full.dtype)
        B = full.numel() // self.world
        lo, hi = (0, B) if lo is None else (lo, hi)
        for q in range(self.world):
            if q != self.rank:
                full[q * B + lo:q * B + hi] = src[q * B + lo:q * B + hi]

    def all_gather(self, full):
        self._fill("all_gather", full)

    def all_gather_async(self, full):
        self._fill("all_gather_async", full)

    def all_gather_piece(self, full, lo, hi):
        self._fill("all_gather_piece", full, lo, hi)

    def _reduce(self, name, t):
        self.calls.append((name, t.data_ptr()))
        if self.force is not None and t.numel() == N.NRED:
            self.force(t)

    def all_reduce_sum(self, t):
        self._reduce("all_reduce_sum", t)

    def all_reduce_sum_async(self, t):
        self._reduce("all_reduce_sum_async", t)


@pytest.mark.parametrize("tiled", [True, False], ids=["tiled", "csr"])
def test_engine_adaptive_retry_gathers_x(tiled):
    """PdlpEngine.adaptive_retry on an engine with a communicator: after pdlp_adaptive_retry it gathers PDLP_BUF_X_CUR, so that the
    K x the next dual half-step recomputes -- from the WHOLE x buffer -- is K x_start and not K times whatever the other ranks'
    blocks held (here 2^60).  Read through the carried K x: pdlp_kkt_local's primal residual after the next iteration."""
    import scipy.sparse as sp
    import torchpdlp_amd as tp
    from torchpdlp_amd.distributed import shard_arrays
    from torchpdlp_amd.tiled import build_tiles
    _ONE.clear()
    gc.collect()
    lp, world, rank = sw.world_lp(), 4, 1
    t = lambda v: torch.tensor(np.asarray(v), dtype=torch.float64, device=DEV)
    args = shard_arrays(sw.csr_pair(lp, torch.float64, DEV), t(lp.c), t(lp.q), t(lp.l), t(lp.u), lp.m_ineq, rank, world, balance="rows")
    part = args.pop("part")
    x0, y0 = hm.start_point(lp, sw.START_SEED)
    xf, yf = part.pad_cols(t(x0)), part.pad_rows(t(y0))
    comm = RecordingComm(rank, world, xf, yf)
    eng = tp.PdlpEngine(comm=comm, **args)
    for tr in (0, 1):
        eng.attach_tiles(tr, None)
        eng.attach_sorted(tr, on=False)
    if tiled:
        lim = eng.tile_limits()
        for tr, (rp, ci, va), rows, cols in ((0, eng.K, eng.ml, eng.n), (1, eng.KT, eng.nl, eng.m)):
            eng.attach_tiles(tr, build_tiles(rp, ci, va, rows, cols, lw=8, rpt=1, groups=1, max_groups=lim["max_groups"],
                                             kernel_limits=(lim["rpt_max"], lim["cap"], lim["nt"])))
        eng.set_exchange_chunks(2)
        assert eng.split_info(0)["local_groups"] > 0
    eng.set_option(N.OPT_RUNNING_KKT, 1)
    (c0, c1), (r0, r1) = eng.cols, eng.rows
    eta0, omega = model().eta0, 1.25
    eng.set_iterate(xf[c0:c1], yf[r0:r1])
    eng.set_step(50.0 * eta0, omega, 1.0, 100000)
    assert torch.equal(eng.buffer(N.BUF_X_CUR), xf) and torch.equal(eng.buffer(N.BUF_Y_CUR), yf)
    for which in (N.BUF_X_CUR, N.BUF_X_PREV, N.BUF_X_AVG):                   # the foreign blocks: not current
        v = eng.buffer(which).view(world, part.Bn)
        v[:rank] = sw.SENTINEL
        v[rank + 1:] = sw.SENTINEL
    # the peers' share of dy'K dx makes eta_bar half the safe step: the trial is rejected, the rule leaves a usable eta'
    def force(red):
        red[2] = (omega * red[0] + red[1] / omega) / (2.0 * 0.5 * eta0)
    comm.force = force
    eng.iterate(1, True)
    comm.force = None
    sc = eng.scalars()
    assert sc["accepted"] == 0 and 0.1 * eta0 < sc["eta"] < eta0, sc
    x_cur = eng.buffer(N.BUF_X_PREV)                     # the buffer that holds the old x: current again after the retry
    comm.calls.clear()
    eng.adaptive_retry()
    assert eng.buffer(N.BUF_X_CUR).data_ptr() == x_cur.data_ptr()
    assert ("all_gather", x_cur.data_ptr()) in comm.calls, comm.calls
    assert torch.equal(eng.buffer(N.BUF_X_CUR), xf)
    eng.iterate(1, True)                                 # its dual half-step recomputes K x of the restored x and carries it on
    x1 = xf.clone()
    x1[c0:c1] = eng.get_iterate(N.CUR)[0]
    N.check(eng.lib.pdlp_kkt_local(eng.h, N.CUR, 0), "pdlp_kkt_local")       # (no gather: the primal side reads the carried K x)
    got = float(eng.buffer(N.BUF_RED)[4])
    Kr = sp.csr_matrix((args["K_rows"][2].cpu().numpy(), args["K_rows"][1].cpu().numpy(), args["K_rows"][0].cpu().numpy()), shape=(eng.ml, eng.n))
    res = Kr @ x1.cpu().numpy() - args["q"].cpu().numpy()
    n_ineq = args["m_ineq"] - r0
    res[:n_ineq] = np.minimum(res[:n_ineq], 0.0)
    want = float(res @ res)
    print(f"primal residual^2 of rank {rank}'s rows from the carried K x: {got!r}, K @ x: {want!r}")
    assert abs(got - want) <= 1e-10 * (1.0 + want)
