"""The constructed matrices of tests/csr_cases.py on the CPU: every case really sits on the limits it is named after (its predicates
hold on the model's schedule, its block, chunk and long-row counts are the stated ones), the model's schedule of a random LP with a
dense row and a dense column has the properties the kernels rely on, ``tiled.sorted_row_blocks`` over the model's blocks marks and
packs them as the format says, and the model decides the adaptive step of the epilogue sequence by a margin no float32 rounding
reaches.  A failing predicate is a broken case: nothing here skips.  (The GPU side: tests/test_gpu_csr_edges.py.)"""
import numpy as np
import pytest
import torch

from tests import csr_cases as cc
from tests import handle_model as hm
from tests import tile_cases as tc
from tests.host_lp import get_lp
from torchpdlp_amd import tiled as T


def test_limits_are_the_library_s():
    assert (cc.BLOCK, cc.NNZ_CAP, cc.ROWS_CAP, cc.MAX_GRID, cc.LONG_GRID, cc.SORT_SHIFT) == (256, 2048, 256, 2048, 64, 21)
    assert cc.NNZ_CAP % cc.BLOCK == 0 and cc.ROWS_CAP <= cc.BLOCK                  # whole item rounds; a lane per row at least
    assert (T.SORTED_MAX_ITEMS, T.SORTED_COL_BITS) == (cc.NNZ_CAP, cc.SORT_SHIFT)
    assert (cc.NNZ_CAP - 1) >> (32 - cc.SORT_SHIFT) == 0                            # every slot of a block fits beside the column bits
    assert [cc.lanes_per_row(k) for k in (1, 3, 4, 5, 8, 9, 129, 256)] == [64, 64, 64, 32, 32, 16, 1, 1]


def _well_formed(rowptr):
    """what the kernels rely on, on the model's schedule of any matrix"""
    rp = np.asarray(rowptr, np.int64)
    s = cc.describe(rp)
    lens = np.diff(rp)
    assert s.blocks[0].tolist() == [0, 0] and s.blocks[-1].tolist() == [rp.size - 1, rp[-1]]
    assert np.all(s.rows >= 1) and np.all(s.rows <= cc.ROWS_CAP) and np.array_equal(s.blocks[:, 1], rp[s.blocks[:, 0]])
    assert np.all((s.items <= cc.NNZ_CAP) | (s.rows == 1))
    # greedy: a block ends at a cap, at the matrix's end, or because the next row does not fit
    for b in range(s.nblk - 1):
        nxt = lens[s.blocks[b + 1, 0]]
        assert s.rows[b] == cc.ROWS_CAP or s.items[b] + nxt > cc.NNZ_CAP
    # long rows: exactly the rows above the cap, each a block by itself, cut into full chunks and a rest of 1 .. NNZ_CAP
    assert s.lrow.tolist() == np.flatnonzero(lens > cc.NNZ_CAP).tolist() == s.blocks[:-1, 0][s.skipped].tolist()
    assert s.lptr[0] == 0 and s.lptr[-1] == s.nchunks and np.all(np.diff(s.lptr) >= 2)
    for i, r in enumerate(s.lrow):
        ch = s.chunks[s.lptr[i]:s.lptr[i + 1]]
        assert ch[0, 0] == rp[r] and ch[-1, 1] == rp[r + 1] and np.array_equal(ch[1:, 0], ch[:-1, 1])
        size = ch[:, 1] - ch[:, 0]
        assert np.all(size[:-1] == cc.NNZ_CAP) and 1 <= size[-1] <= cc.NNZ_CAP
    return s


@pytest.mark.parametrize("name", cc.NAMES)
def test_case_holds_its_edge(name):
    case = cc.get_case(name)
    A = case.A
    assert np.array_equal(A.data, A.data.astype(np.float32).astype(np.float64)) and A.has_sorted_indices and A.indices.dtype == np.int32
    assert all(np.all(np.diff(A.indices[a:e]) > 0) for a, e in zip(A.indptr[:-1], A.indptr[1:]) if e - a > 1)
    assert cc.broken_predicates(name) == []
    s, t = _well_formed(A.indptr), _well_formed(A.T.tocsr().indptr)
    assert dict(rows=A.shape[0], items=A.nnz, blocks=s.nblk, chunks=s.nchunks, long=s.nlong) == case.counts
    assert np.array_equal(s.blocks, cc.get_sched(name, "K")[0].blocks) and np.array_equal(t.blocks, cc.get_sched(name, "KT")[0].blocks)


def test_row_length_lists_give_the_stated_counts():
    """the table of the cases, from the row lengths alone"""
    rp = lambda lengths: np.concatenate([[0], np.cumsum(lengths)])
    s = cc.describe(rp(cc.LONG_LENGTHS))
    assert (s.nblk, s.nchunks, s.nlong, s.grid, s.lgrid) == (13, 60, 8, 73, 1)
    assert sorted(np.diff(s.lptr).tolist()) == [2, 2, 2, 3, 8, 9, 17, 17]
    s = cc.describe(rp([1025] * 700 + [2049] + [1025] * 799 + [6146] + [1025] * 599 + [2049] * 300))
    assert (s.nblk, s.nchunks, s.nlong, s.grid, s.lgrid) == (2400, 606, 302, cc.MAX_GRID, 2)
    s = cc.describe(rp([8] * 256 + [0] * 356 + [5] * 30 + [0] * 3))
    assert (s.nblk, s.nchunks, s.nlong, s.grid, s.lgrid) == (3, 0, 0, 3, 0)
    assert cc.describe(rp([])).nblk == 0 and cc.describe(rp([0])).rows.tolist() == [1]
    assert cc.describe(rp([cc.NNZ_CAP])).nlong == 0 and cc.describe(rp([cc.NNZ_CAP + 1])).chunks.tolist() == [[0, cc.NNZ_CAP], [cc.NNZ_CAP, cc.NNZ_CAP + 1]]


def test_schedule_of_a_random_lp_with_a_dense_row_and_column():
    lp = get_lp("long")                                      # sparse_lp(2500, 2300, 3, 7, dense=True)
    for A, dense in ((lp.A, 2500 // 3), (lp.A.T.tocsr(), 2300 // 2)):
        s = _well_formed(A.indptr)
        assert s.lrow.tolist() == [dense] and s.nchunks == 2 and s.lgrid == 1 and s.grid == s.nblk + 2
        assert s.chunks[0, 1] - s.chunks[0, 0] == cc.NNZ_CAP and s.chunks[1, 1] - s.chunks[1, 0] == A.shape[1] - cc.NNZ_CAP


@pytest.mark.parametrize("side", ["K", "KT"])
@pytest.mark.parametrize("name", cc.NAMES)
def test_sorted_row_blocks_over_the_model_s_blocks(name, side):
    """cbase >= 0 exactly where the format allows a sorted block; there the words decode, as unsigned numbers, to a permutation of
    the block's slots with each slot's own column and value, in ascending column order"""
    A = cc.get_case(name).A
    A = A.T.tocsr() if side == "KT" else A
    A.sort_indices()
    s, indices = cc.get_sched(name, side)
    first = s.blocks[:, 1]
    sidx, sval, cbase, n_sorted = T.sorted_row_blocks(torch.from_numpy(first.copy()), torch.from_numpy(A.indices.copy()),
                                                      torch.from_numpy(A.data.astype(np.float32)))
    want = cc.sortable(s.blocks, indices)
    assert n_sorted == int(want.sum()) == cc.n_sorted(name, side)
    cbase = cbase.numpy()
    assert np.array_equal(cbase >= 0, want) and np.all(cbase[~want] == -1)
    if name == "sorted_limits" and side == "K":
        assert want.tolist() == cc.SORTED_PATTERN
    word = sidx.numpy().astype(np.int64) & 0xFFFFFFFF
    slot, off = word >> cc.SORT_SHIFT, word & ((1 << cc.SORT_SHIFT) - 1)
    sval, val32 = sval.numpy(), A.data.astype(np.float32)
    top_bit = False
    for b in np.flatnonzero(want):
        a, e = first[b], first[b + 1]
        assert np.array_equal(np.sort(slot[a:e]), np.arange(e - a)), b
        col = cbase[b] + off[a:e]
        assert np.array_equal(col, A.indices[a + slot[a:e]]) and np.all(np.diff(col) >= 0) and cbase[b] == A.indices[a:e].min(), b
        assert np.array_equal(sval[a:e], val32[a + slot[a:e]]), b
        top_bit = top_bit or bool((sidx.numpy()[a:e] < 0).any())
    if name in ("ladder", "sorted_limits") and side == "K":
        assert top_bit, "no slot from 1024 on: bit 31 is never set"


@pytest.mark.parametrize("side", ["K", "KT"])
@pytest.mark.parametrize("name", cc.NAMES)
def test_adaptive_step_of_the_sequence_is_decided(name, side):
    """the epilogue check walks one adaptive step: the model must accept or reject it by a margin no rounding of a float32 engine
    reaches, |eta - eta_bar| / eta_bar > 1e-2; and the iterates stay of order 1 (the step is 0.5 / ||K||)"""
    lp = cc.get_lp(name, side)
    assert lp.m_ineq == 2 * lp.m // 5 and np.isinf(lp.l).any() and np.isinf(lp.u).any() and (lp.l == lp.u).any()
    model = hm.HandleModel(lp)
    for call in cc.SEQUENCE:
        if call[0] == "iterate" and call[2]:
            eta = model.eta
            _, _, _, _, info = model.o.step_adaptive(model.x, model.y, model.eta, model.omega, model.theta, model.k + 1)
            margin = abs(eta - info["eta_bar"]) / info["eta_bar"]
            print(f"{name} {side}: margin {margin:.4f}, ||K|| {lp.norm2():.1f}")
            assert margin > 1e-2, (margin, eta, info)
        model.apply(call)
        if call[0] == "set_step":
            assert abs(model.eta * lp.norm2() - 0.5) < 1e-12
    assert model.k == 2 and model.xp is not None
    assert max(np.abs(model.x).max(), np.abs(model.y).max()) < 50.0


def test_exact_product_fast_path():
    """rows of no or one item skip ``math.fsum``: the same numbers as the sums"""
    import math
    A = cc.from_lengths([0, 1, 2, 5, 1, 0, 3, 40], 50, 3)
    v = tc.probe(A.shape[1])
    ref, mag, items = tc.exact_product(A, v)
    assert {0, 1} <= set(items.tolist()) and items.max() > 1
    for r in range(A.shape[0]):
        p = A.data[A.indptr[r]:A.indptr[r + 1]] * v[A.indices[A.indptr[r]:A.indptr[r + 1]]]
        assert ref[r] == math.fsum(p) and mag[r] == math.fsum(np.abs(p))
