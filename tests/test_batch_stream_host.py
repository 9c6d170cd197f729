"""CPU checks of the streamed batch (``solve_lp_batch(slots=...)``): the C ABI of its three entry points, the queue that hands the
columns out, and the argument checks that come before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import torchpdlp_amd as tp
from torchpdlp_amd import _native as N
from torchpdlp_amd import batch as tb
from torchpdlp_amd.rules import StreamQueue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pdlp_hip.h")
NEW = ("pdlp_batch_iterate_from", "pdlp_batch_admit", "pdlp_batch_retire")


def header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_exports_and_binding_agree_on_the_new_entry_points():
    src = header()
    lib = C.CDLL(N.LIB_PATH)
    for name in NEW:
        decl = re.search(r"\bint " + name + r"\s*\(([^)]*)\)", src)
        assert decl, f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in N.SIGNATURES
        assert len(N.SIGNATURES[name][1]) == len(decl.group(1).split(",")), name
    # the pinned layout is untouched: the new state travels as arguments and in a struct of its own
    assert N.ABI_VERSION == 18 and N.load().pdlp_abi_version() == 18
    assert len(N.PdlpBatch._fields_) == 31


def test_feed_struct_matches_the_header():
    body = re.search(r"typedef struct pdlp_batch_feed \{(.*?)\} pdlp_batch_feed;", header(), flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [d.strip().split()[-1].lstrip("*") for d in decl.split(",")]
    assert names == [f[0] for f in N.PdlpBatchFeed._fields_]
    assert N.PdlpBatchFeed._fields_[0][1] is C.c_int32
    assert all(ty is C.c_void_p for _, ty in N.PdlpBatchFeed._fields_[1:])


def test_null_handles_are_rejected_without_a_gpu():
    lib = N.load()
    b, f = N.PdlpBatch(), N.PdlpBatchFeed()
    assert lib.pdlp_batch_iterate_from(None, C.byref(b), 1, 0, 0, None) == -1
    assert lib.pdlp_batch_admit(None, C.byref(b), 1, None, None, C.byref(f)) == -1
    assert lib.pdlp_batch_retire(None, C.byref(b), 1, None, None, N.CUR, 0, 0, None, None, None, None, 1) == -1
    assert lib.pdlp_batch_iterate_from(None, None, 1, 0, 0, None) == -1
    assert lib.pdlp_batch_iterate_from(None, C.byref(b), -1, 0, 0, None) == -1 and lib.pdlp_batch_iterate_from(None, C.byref(b), 1, 0, -1, None) == -1
    assert lib.pdlp_batch_retire(None, C.byref(b), 1, None, None, 7, 0, 0, None, None, None, None, 1) == -1     # bad iterate code
    assert lib.pdlp_batch_retire(None, C.byref(b), 1, None, None, N.CUR, 0, 3, None, None, None, None, 1) == -1  # bad slot


def simulate(B, slots, period, finish_after, segments, time_cut=None):
    """drive the queue the way ``_solve_stream`` does.  LP i finishes ``finish_after[i]`` checks of its own after its admission;
    ``segments(k)`` gives the length of the next segment at count k (a cap inside a period cuts one short).  ``time_cut``: the
    count at which the clock runs out.  Returns the queue and the log of (event, k_global, column, lp)."""
    q = StreamQueue(B, slots, period)
    log, k, left = [], 0, np.zeros(slots, np.int64)

    def admit():
        cols, ids = q.admit(k)
        for c_, i in zip(cols, ids):
            left[c_] = finish_after[i]
            log.append(("admit", k, int(c_), int(i)))

    admit()
    while q.occupied().size:
        live = q.occupied()[left[q.occupied()] > 0]
        cut = time_cut is not None and k >= time_cut
        if live.size and not cut:
            k += segments(k)
            if k % period == 0:
                left[live] -= 1
        if cut or not live.size:
            left[:] = 0
            k = q.next_boundary(k)
        if q.may_admit(k):
            done = q.occupied()[left[q.occupied()] <= 0]
            for c_, i in zip(done, q.retire(done, k)):
                log.append(("retire", k, int(c_), int(i)))
            if not cut:
                admit()
    return q, log


def test_queue_admits_every_lp_once_in_order_at_check_boundaries():
    B, slots, period = 50, 8, 40
    rng = np.random.default_rng(5)
    finish_after = rng.integers(1, 7, B)
    finish_after[::3] = 1                                        # every third LP is done at its first check
    # a KKT-pass cap inside a period: some segments stop short of the boundary, the next one completes the period
    segments = lambda k: (13 if k % period == 0 and (k // period) % 3 == 1 else period - k % period)
    q, log = simulate(B, slots, period, finish_after, segments)
    admits = [e for e in log if e[0] == "admit"]
    retires = [e for e in log if e[0] == "retire"]
    assert [e[3] for e in admits] == list(range(B))              # once each, in index order
    assert all(e[1] % period == 0 for e in admits)               # only at a check of the batch
    assert sorted(e[3] for e in retires) == list(range(B))       # every LP leaves
    holder = {}
    for ev, k, col, lp in log:                                   # no column ever holds two LPs
        if ev == "admit":
            assert col not in holder, (col, lp, holder)
            holder[col] = lp
        else:
            assert holder.pop(col) == lp
    assert not holder and not q.waiting() and not q.occupied().size
    # each LP ran finish_after[i] periods in its column; the schedule says where and when
    s = q.schedule()
    assert ((s["retired_at"] - s["admitted_at"]) >= finish_after * period).all()
    assert (s["column"] >= 0).all() and (s["column"] < slots).all()
    assert (s["admitted_at"][:slots] == 0).all() and s["admitted_at"].max() > 0
    with pytest.raises(ValueError):
        StreamQueue(4, 2, 40).admit(13)                          # not at a boundary
    with pytest.raises(ValueError):
        q.retire([0], 0)                                         # an empty column


def test_queue_reports_the_lps_a_time_limit_cuts_off():
    B, slots, period = 50, 8, 40
    finish_after = np.full(B, 3)
    q, log = simulate(B, slots, period, finish_after, lambda k: period - k % period, time_cut=200)
    admitted = sorted(e[3] for e in log if e[0] == "admit")
    late = q.never_admitted()
    assert len(admitted) + late.size == B and late.size > 0
    assert list(late) == list(range(len(admitted), B))
    s = q.schedule()
    assert (s["admitted_at"][late] == -1).all() and (s["column"][late] == -1).all() and (s["retired_at"][late] == -1).all()
    assert (s["retired_at"][admitted] >= 0).all()                # those that ran were all taken out


def lp_family(B):
    f = tp.gen_lp_family(30, 24, 3, B, seed=1)
    return f, tp.CsrPair(f.m, f.n, f.rowptr, f.colidx, f.val)


class NoDevice:
    def __init__(self, *a, **kw):
        raise AssertionError("the argument check must come before any device work")


@pytest.mark.parametrize("kw", [dict(slots=12), dict(slots=0), dict(slots=8, K_values=True, precondition=True),
                                dict(slots=16, group_width=32), dict(slots=-8)])
def test_bad_slots_raise_before_device_work(monkeypatch, kw):
    monkeypatch.setattr(tb, "BatchEngine", NoDevice)
    f, K = lp_family(20)
    kw = dict(kw)
    if kw.pop("K_values", False):
        kw["K_values"] = K.val.view(-1, 1).repeat(1, 20)
    with pytest.raises(ValueError):
        tp.solve_lp_batch((f.C[:, 0], K, f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0]), f.C, f.Q, f.L, f.U, device="cuda", **kw)
    solver_kw = dict(kw)
    if solver_kw.pop("precondition", False):
        solver_kw.update(precondition=True, data_precond=(torch.ones(f.n, 20), torch.ones(f.m, 20)))
    with pytest.raises(ValueError):
        tb.pdlp_algorithm_batch(K, f.m_ineq, f.C, f.Q, f.L, f.U, "cuda", sigma=1.0, **solver_kw)


def test_unsupported_flags_still_raise_when_streamed():
    f, K = lp_family(20)
    for flag in ("comm", "fishnet", "infeasibility_detect", "adaptive_retry", "direct_exchange"):
        with pytest.raises(ValueError, match="no batched form"):
            tp.solve_lp_batch((f.C[:, 0], K, f.Q[:, 0], f.m_ineq, f.L[:, 0], f.U[:, 0]), f.C, f.Q, f.L, f.U, slots=8, **{flag: True})
