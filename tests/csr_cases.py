"""Constructed matrices that sit on the limits of the CSR kernels' schedule (k_csr_fused, its SORTED form and k_long_rows in
csrc/pdlp_kernel_csr.inc; build_schedule_host and build_long_rows_host in csrc/pdlp_schedule.inc; ``tiled.sorted_row_blocks``), and
a model of that schedule.  Host only: numpy, scipy.

The model is written from the description of the format, not by calling the library:

  * a row block is the longest run of consecutive rows that holds at most ``NNZ_CAP`` items and at most ``ROWS_CAP`` rows (rows
    without items ride along for as long as the row cap allows); a single row of more than ``NNZ_CAP`` items is a block by itself,
    which the block loop skips;
  * such a LONG row is cut into chunks of ``NNZ_CAP`` items (the last one holds the rest, 1 .. ``NNZ_CAP``); blocks and chunks share
    one index space of work items, blocks first, of which ``min(blocks + chunks, MAX_GRID)`` workgroups each take every grid-th;
  * ``k_long_rows`` gives every long row one thread: ``min(ceil(long rows / BLOCK), LONG_GRID)`` workgroups, whose partial sums stand
    behind the block kernel's;
  * a block of ``nrows`` rows gives each row ``min(64, 2^floor(log2(BLOCK / nrows)))`` lanes;
  * the sorted form packs ``slot << SORT_SHIFT | column - cbase`` into one 32-bit word (slots from 1024 on set bit 31); a block
    without items, of more than ``NNZ_CAP`` items or whose columns span ``2^SORT_SHIFT`` or more keeps CSR order (``cbase = -1``).

A case is built from a list of row lengths (or, for ``sorted_limits``, of explicit columns) with distinct ascending columns in every
row, and carries PREDICATES on the model's schedule of the matrix and of its transpose that say the edge it is named after is really
there.  A predicate that fails is a broken case, never a reason to skip.  Every case is used as K and, transposed, as K'
(``get_lp``).  tests/test_csr_cases_host.py checks the cases on the CPU, tests/test_gpu_csr_edges.py runs them."""
from collections import namedtuple
from dataclasses import dataclass, field
import os
import re

import numpy as np
import scipy.sparse as sp

from tests import tile_cases as tc

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "torchpdlp_amd", "csrc")


def _constant(file, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(_CSRC, file)).read()).group(1))


BLOCK, NNZ_CAP, ROWS_CAP, MAX_GRID = (_constant("pdlp_hip.hip", k) for k in ("BLOCK", "NNZ_CAP", "ROWS_CAP", "MAX_GRID"))
LONG_GRID = _constant("pdlp_handle.inc", "LONG_GRID")
SORT_SHIFT = _constant("pdlp_kernel_csr.inc", "SORT_SHIFT")
LONG_ROUND = 8                       # chunk sums that long_pass adds per round trip
NAMES = ("ladder", "full_and_empty", "long_rows", "grid_stride", "sorted_limits")
LADDER = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)


# ---- the model of the schedule -----------------------------------------------------------------------------------------
def schedule(rowptr):
    """[(first row, first item)] of every block, then (rows, items) as the end marker: an int64 array of shape (blocks + 1, 2)"""
    rp = np.asarray(rowptr, np.int64)
    rows = rp.size - 1
    out, r = [(0, 0)], 0
    while r < rows:
        fits = int(np.searchsorted(rp, rp[r] + NNZ_CAP, side="right")) - 1        # the last e with rp[e] - rp[r] <= NNZ_CAP
        e = max(min(fits, r + ROWS_CAP, rows), r + 1)                             # (a longer single row: a block by itself)
        out.append((e, int(rp[e])))
        r = e
    return np.array(out, np.int64).reshape(-1, 2)


def long_rows(rowptr):
    """(chunks [(first item, end)], long rows, chunk range of every long row [long rows + 1])"""
    rp = np.asarray(rowptr, np.int64)
    lens = np.diff(rp)
    rows = np.flatnonzero(lens > NNZ_CAP)
    chunks, ptr = [], [0]
    for r in rows:
        a, e = int(rp[r]), int(rp[r + 1])
        chunks += [(c, min(c + NNZ_CAP, e)) for c in range(a, e, NNZ_CAP)]
        ptr.append(len(chunks))
    return np.array(chunks, np.int64).reshape(-1, 2), rows.astype(np.int64), np.array(ptr, np.int64)


def lanes_per_row(nrows):
    return min(64, 1 << int(np.floor(np.log2(BLOCK // nrows))))


Sched = namedtuple("Sched", "blocks chunks lrow lptr nblk nchunks nlong grid lgrid rows items skipped")


def describe(rowptr):
    """the schedule of one matrix with everything the predicates look at: ``rows`` / ``items`` per block, ``skipped`` = the blocks
    that are one long row, ``grid`` / ``lgrid`` = the workgroups of k_csr_fused / k_long_rows"""
    blocks = schedule(rowptr)
    chunks, lrow, lptr = long_rows(rowptr)
    nblk, nchunks, nlong = blocks.shape[0] - 1, chunks.shape[0], lrow.size
    items = np.diff(blocks[:, 1])
    return Sched(blocks, chunks, lrow, lptr, nblk, nchunks, nlong, min(nblk + nchunks, MAX_GRID), min(-(-nlong // BLOCK), LONG_GRID),
                 np.diff(blocks[:, 0]), items, items > NNZ_CAP)


def sortable(blocks, indices):
    """per block: does the sorted form read its column-sorted copy (``cbase >= 0``)?  Items in 1 .. NNZ_CAP, columns spanning less than
    2^SORT_SHIFT"""
    first = blocks[:, 1]
    ok = np.zeros(first.size - 1, bool)
    for b in np.flatnonzero((np.diff(first) > 0) & (np.diff(first) <= NNZ_CAP)):
        c = indices[first[b]:first[b + 1]]
        ok[b] = int(c.max()) - int(c.min()) < (1 << SORT_SHIFT)
    return ok


def spans(blocks, indices):
    """largest minus smallest column of every block (-1: no items)"""
    first = blocks[:, 1]
    return np.array([int(indices[a:e].max()) - int(indices[a:e].min()) if e > a else -1 for a, e in zip(first[:-1], first[1:])], np.int64)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    A: sp.csr_matrix                   # float64 whose every value is a float32 number
    counts: dict                       # blocks, chunks and long rows of A: the table of the cases, stated and not computed
    predicates: list = field(default_factory=list)     # (what, function of (Sched of A, Sched of A', Case) -> bool)


def from_lengths(lengths, ncols, seed):
    """CSR with ``lengths[r]`` items in row r at distinct ascending columns"""
    lw = max(1, int(np.ceil(np.log2(ncols))))
    return tc.matrix_from_counts(np.asarray(lengths, np.int64).reshape(-1, 1), lw, ncols, seed)


def _draw(rng, lo, hi, k, first=None, last=None):
    """k distinct ascending columns of [lo, hi): one at a random place of each of k equal strata; ``first`` / ``last`` replace the
    ends (with columns that may lie outside [lo, hi))"""
    if k == 0:
        return np.zeros(0, np.int64)
    j, w = np.arange(k, dtype=np.int64), hi - lo
    a, e = j * w // k, (j + 1) * w // k
    col = lo + a + np.minimum((rng.random(k) * (e - a)).astype(np.int64), e - a - 1)
    if first is not None:
        col[0] = first
    if last is not None:
        col[-1] = last
    assert np.all(np.diff(col) > 0)
    return col


def from_columns(rows, ncols, seed):
    """CSR whose row r holds the ascending distinct columns ``rows[r]``"""
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int64)
    col = np.concatenate([np.asarray(c, np.int64) for c in rows]) if len(rows) else np.zeros(0, np.int64)
    val = tc._f32(rng.standard_normal(col.size))
    val[val == 0] = 1.0
    assert all(np.all(np.diff(c) > 0) for c in rows if len(c) > 1)
    return sp.csr_matrix((val, col.astype(np.int32), indptr), shape=(len(rows), ncols))


def ladder():
    """22 blocks of exactly k rows and exactly NNZ_CAP items, k over ``LADDER``: every lane count from 1 to 64, idle lanes for
    every k that is no power of two"""
    lengths = []
    for k in LADDER:
        lengths += [NNZ_CAP - (k - 1)] + [1] * (k - 1)
    return Case("ladder", from_lengths(lengths, 2500, 11), dict(rows=1270, items=45056, blocks=22, chunks=0, long=0), [
        ("the blocks hold k rows each, k over the ladder", lambda s, t, c: s.rows.tolist() == list(LADDER)),
        ("every block holds exactly NNZ_CAP items", lambda s, t, c: bool(np.all(s.items == NNZ_CAP)) and not s.skipped.any()),
        ("every lane count from 1 to 64 occurs", lambda s, t, c: {lanes_per_row(k) for k in s.rows} == {1, 2, 4, 8, 16, 32, 64}),
        ("most row counts leave lanes idle", lambda s, t, c: sum(lanes_per_row(k) * k < BLOCK for k in s.rows) >= 12),
    ])


def full_and_empty():
    """a block at both caps at once, a block without an item, empty rows at a block's start and at the matrix's end"""
    lengths = [8] * 256 + [0] * 256 + [0] * 100 + [5] * 30 + [0] * 3
    return Case("full_and_empty", from_lengths(lengths, 300, 12), dict(rows=645, items=2198, blocks=3, chunks=0, long=0), [
        ("block 0 is at the row cap and the item cap at once", lambda s, t, c: (s.rows[0], s.items[0]) == (ROWS_CAP, NNZ_CAP)),
        ("block 1 is ROWS_CAP rows without an item", lambda s, t, c: (s.rows[1], s.items[1]) == (ROWS_CAP, 0)),
        ("block 2 starts with 100 empty rows and ends the matrix with 3", lambda s, t, c: (s.rows[2], s.items[2]) == (133, 150) and
         np.diff(c.A.indptr)[512:612].max() == 0 and np.diff(c.A.indptr)[-3:].max() == 0 and np.diff(c.A.indptr)[-4] == 5),
    ])


LONG_LENGTHS = [2049, 0, 4096, 4097, 3, 16384, 16385, 0, 0, 32773, 34816, 4, 2048, 2049]


def long_rows_case():
    """8 long rows in 60 chunks: last chunks of 1 and of 5 items, rows of exactly 2, 8, 9 and 17 chunks (k_long_rows adds eight at a
    time), a long row first and last, long rows side by side and beside empty rows, a row of exactly NNZ_CAP items that is not long"""
    per_row = lambda s: np.diff(s.lptr).tolist()
    tails = lambda s: (s.chunks[s.lptr[1:] - 1, 1] - s.chunks[s.lptr[1:] - 1, 0]).tolist()
    return Case("long_rows", from_lengths(LONG_LENGTHS, 34856, 13), dict(rows=14, items=sum(LONG_LENGTHS), blocks=13, chunks=60, long=8), [
        ("long rows 0, 2, 3, 5, 6, 9, 10, 13", lambda s, t, c: s.lrow.tolist() == [0, 2, 3, 5, 6, 9, 10, 13]),
        ("of 2, 2, 3, 8, 9, 17, 17 and 2 chunks", lambda s, t, c: per_row(s) == [2, 2, 3, 8, 9, 17, 17, 2]),
        ("last chunks of 1, 2048, 1, 2048, 1, 5, 2048 and 1 items", lambda s, t, c: tails(s) == [1, NNZ_CAP, 1, NNZ_CAP, 1, 5, NNZ_CAP, 1]),
        ("chunk counts of 8k, 8k + 1 and fewer than 8", lambda s, t, c: {n % LONG_ROUND for n in per_row(s)} >= {0, 1, 2, 3}),
        ("every long row is a block by itself, the block loop skips exactly those",
         lambda s, t, c: s.blocks[:-1, 0][s.skipped].tolist() == s.lrow.tolist() and bool(np.all(s.rows[s.skipped] == 1))),
        ("the row of exactly NNZ_CAP items is a block, not a long row",
         lambda s, t, c: 12 in s.blocks[:, 0].tolist() and s.items[s.blocks[:-1, 0].tolist().index(12)] == NNZ_CAP and 12 not in s.lrow.tolist()),
        ("a block of two rows without items stands between long rows", lambda s, t, c: [7, 0] in np.stack([s.blocks[:-1, 0], s.items], 1).tolist()),
    ])


def grid_stride():
    """blocks + chunks > MAX_GRID: workgroups take a second work item, of the blocks and of the chunks; 302 long rows: a second
    workgroup of k_long_rows, whose partial sums stand in the slot behind the first's"""
    lengths = [1025] * 2100
    lengths[700], lengths[1500] = 2049, 6146
    lengths += [2049] * 300
    return Case("grid_stride", from_lengths(lengths, 7000, 14), dict(rows=2400, items=2773345, blocks=2400, chunks=606, long=302), [
        ("every row is a block", lambda s, t, c: bool(np.all(s.rows == 1))),
        ("more blocks than workgroups: blocks stride", lambda s, t, c: s.nblk > MAX_GRID == s.grid),
        ("every chunk is the second work item of its workgroup, behind a block", lambda s, t, c: MAX_GRID < s.nblk < s.nblk + s.nchunks <= 2 * MAX_GRID),
        ("long rows of 2 and of 4 chunks among the blocks", lambda s, t, c: s.lrow[:2].tolist() == [700, 1500] and np.diff(s.lptr)[:2].tolist() == [2, 4]),
        ("a second workgroup of k_long_rows", lambda s, t, c: s.nlong > BLOCK and s.lgrid == 2),
        ("the transpose has no long row", lambda s, t, c: t.nlong == 0 and t.nblk > 1),
    ])


SORTED_WIDE = 1 << 21
SORTED_N = SORTED_WIDE + 64
SORTED_PATTERN = [True, False, True, False, True, False, True]        # which blocks the sorted form reads sorted


def sorted_limits():
    """the limits of the sorted form's 32-bit word: a block 2^21 - 1 columns wide (sorted) and one 2^21 wide (CSR order), a block of
    exactly NNZ_CAP items over several rows (slots up to 2047: bit 31), a long row between two sorted blocks, an all-empty block, two
    rows of one block that share columns; the transpose: 2 097 216 rows in 8193 blocks, nearly all of them without items"""
    rng = np.random.default_rng(15)
    n, W = SORTED_N, SORTED_WIDE
    rows = []
    # (all but the first and last column of a wide block stand in a band of 8192 columns: the transpose's blocks stay empty)
    # block 0: 4 x 512 items, the first at column 0 and the last at column 2^21 - 1; the last row's 512 stand in the top band, so a
    # quarter of the block's column offsets use bit 20
    for r in range(4):
        lo = W - 8192 if r == 3 else 1000
        rows.append(_draw(rng, lo, lo + 8192, 512, first=0 if r == 0 else None, last=W - 1 if r == 3 else None))
    # block 1: 700 + 700 + 648 items, the first at column 10 and the last at column 10 + 2^21
    for r, k in enumerate((700, 700, 648)):
        rows.append(_draw(rng, 20000, 20000 + 8192, k, first=10 if r == 0 else None, last=10 + W if r == 2 else None))
    # block 2: NNZ_CAP items in 7 rows (one of them empty) of a band of 4096 columns; row 0's columns are among row 3's
    shared = _draw(rng, 5000, 5000 + 4096, 500)
    for r, k in enumerate((300, 1, 0, 500, 247, 999, 1)):
        rows.append(np.sort(rng.choice(shared, 300, replace=False)) if r == 0 else shared if r == 3 else _draw(rng, 5000, 5000 + 4096, k))
    # block 3: a long row of 3 chunks
    rows.append(_draw(rng, 200000, 220000, 5000))
    # block 4: 20 rows of 10 items and 236 rows without (the row cap ends it); block 5: ROWS_CAP rows without items
    rows += [_draw(rng, 100000, 100400, 10) for _ in range(20)] + [np.zeros(0, np.int64)] * (236 + ROWS_CAP)
    # block 6: the last columns of the matrix
    rows += [_draw(rng, n - 40, n, 3, last=n - 1 if r == 4 else None) for r in range(5)]
    items = [NNZ_CAP, NNZ_CAP, NNZ_CAP, 5000, 200, 0, 15]
    share = lambda c: np.intersect1d(c.A.indices[c.A.indptr[7]:c.A.indptr[8]], c.A.indices[c.A.indptr[10]:c.A.indptr[11]]).size
    return Case("sorted_limits", from_columns(rows, n, 16), dict(rows=532, items=sum(items), blocks=7, chunks=3, long=1), [
        ("seven blocks of 2048, 2048, 2048, 5000, 200, 0 and 15 items", lambda s, t, c: s.items.tolist() == items),
        ("of 4, 3, 7, 1, 256, 256 and 5 rows", lambda s, t, c: s.rows.tolist() == [4, 3, 7, 1, ROWS_CAP, ROWS_CAP, 5]),
        ("block 0 spans exactly 2^21 - 1 columns, block 1 exactly 2^21", lambda s, t, c: spans(s.blocks, c.A.indices)[:2].tolist() == [W - 1, W]),
        ("512 column offsets of block 0 use the top bit of the column field", lambda s, t, c: int((c.A.indices[:NNZ_CAP] >= W // 2).sum()) == 512),
        ("blocks 0, 2, 4 and 6 are read sorted", lambda s, t, c: sortable(s.blocks, c.A.indices).tolist() == SORTED_PATTERN),
        ("the long row stands between two sorted blocks", lambda s, t, c: s.skipped.tolist() == [False] * 3 + [True] + [False] * 3 and s.lrow.tolist() == [14]),
        ("rows 7 and 10 (block 2) share 300 columns", lambda s, t, c: share(c) == 300),
        ("the last block reaches the last column", lambda s, t, c: int(c.A.indices.max()) == n - 1 == int(c.A.indices[-1])),
        ("the transpose: 8193 blocks of ROWS_CAP rows, four times MAX_GRID", lambda s, t, c: t.nblk == 8193 > 4 * MAX_GRID and t.grid == MAX_GRID and t.nlong == 0),
        ("nearly all of them without an item", lambda s, t, c: int((t.items == 0).sum()) > 8000),
    ])


_MAKERS = dict(ladder=ladder, full_and_empty=full_and_empty, long_rows=long_rows_case, grid_stride=grid_stride, sorted_limits=sorted_limits)
_CASES, _SCHED, _LPS, _REF = {}, {}, {}, {}


def get_case(name):
    """built once per session, shared, never written to"""
    if name not in _CASES:
        _CASES[name] = _MAKERS[name]()
    return _CASES[name]


def get_sched(name, side="K"):
    """the model's schedule of the case matrix ("K") or of its transpose ("KT"), with the transposed matrix's column indices"""
    if (name, side) not in _SCHED:
        A = get_case(name).A
        A = A.T.tocsr() if side == "KT" else A
        A.sort_indices()
        _SCHED[name, side] = (describe(A.indptr), A.indices)
    return _SCHED[name, side]


def broken_predicates(name):
    case = get_case(name)
    s, t = get_sched(name, "K")[0], get_sched(name, "KT")[0]
    return [what for what, holds in case.predicates if not holds(s, t, case)]


def n_sorted(name, side):
    """blocks of the case matrix ("K") or its transpose ("KT") that the sorted form reads sorted"""
    s, indices = get_sched(name, side)
    return int(sortable(s.blocks, indices).sum())


def params():
    """(case, precision, side, form) of every GPU test"""
    return [(n, p, s, f) for n in NAMES for p in tc.LIMITS for s in ("K", "KT") for f in ("csr", "sorted")]


# ---- the reference of the product and the LP around a case ---------------------------------------------------------------------
def reference(name, of="K"):
    """(probe vector, exact row sums, sum |K||v|, items per row) of the case matrix ("K") or of its transpose ("KT"): computed
    once, shared, never written to"""
    if (name, of) not in _REF:
        A = get_case(name).A
        A = A.T.tocsr() if of == "KT" else A
        A.sort_indices()
        v = tc.probe(A.shape[1], 5 if of == "K" else 6)
        _REF[name, of] = (v,) + tc.exact_product(A, v)
        for a in _REF[name, of]:
            a.setflags(write=False)
    return _REF[name, of]


# tile_cases' sequence with the fixed step at eta = 0.5 / ||K||_2 (the model's set_step takes a factor on 0.9 / ||K||_2): with it
# the iterates stay of order 1 on both sides of ``long_rows`` (||K|| about 186)
SEQUENCE = [("set_step", 0.5 / 0.9) + c[2:] if c[0] == "set_step" else c for c in tc.SEQUENCE]
LP_SEED = dict(ladder=950, full_and_empty=951, long_rows=952, grid_stride=953, sorted_limits=954)


def get_lp(name, side):
    """HostLP whose K (side "K") or K' (side "KT") is the case matrix: all four bound classes, m_ineq = 2m/5 as ``tile_cases.get_lp``"""
    from tests.host_lp import HostLP, _bounds
    if (name, side) not in _LPS:
        A = get_case(name).A
        A = A.T.tocsr() if side == "KT" else A
        m, n = A.shape
        rng = np.random.default_rng(LP_SEED[name])
        l, u = _bounds(rng, n, True)
        lp = HostLP(A, (2 * m) // 5, rng.standard_normal(n), rng.standard_normal(m), l, u)
        norm = lp.norm2()
        lp.norm2 = lambda: norm                              # (40 products of the largest case: once per LP, not once per model)
        _LPS[name, side] = lp
    return _LPS[name, side]
