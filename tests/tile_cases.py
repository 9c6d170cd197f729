"""Constructed matrices that sit on the limits of the panel-tiled format (torchpdlp_amd/tiled.py), for the kernel that reads it
(k_tiled_fused, k_rowsum_epilogue, k_rem_segments, k_rem_rows in csrc/pdlp_kernel_tiled.inc).  Host only: numpy, scipy, torch on the CPU.

A case is a function of the limits of one kernel instantiation.  It fixes a row-count array ``cnt[row][panel]`` first and then draws
that many distinct, ascending columns inside every panel, so what a tile holds is known before ``build_tiles`` runs.  A case carries
the ``build_tiles`` arguments, the panel-group counts it is run with and its EDGE PREDICATES: conditions on the built ``Tiles`` (through
``tile_row_counts``, ``tile_ptr``, ``rem_rptr``, ``rem_sptr``) that say the edge the case is named after is really there.  A predicate
that fails is a broken case, never a reason to skip.

Every case is used as it stands (the edge in K) and transposed (the engine's matrix is the case's transpose, so the case matrix is K'
and the primal-side epilogues run over the edge).  The other side of either engine is tiled with the same ``lw`` / ``rpt`` /
``max_rest`` where ``build_tiles`` can (``Case.other_side_csr``: where it cannot, that side stays with the CSR kernel).

``remainder_tails`` is not in the list the tests were first drawn up from: it was added for three mutants of the kernels that the
listed ``remainder`` case cannot see (profiles/r16_tile_edges/README.md)."""
from collections import namedtuple
from dataclasses import dataclass, field
import math

import numpy as np
import scipy.sparse as sp
import torch

from torchpdlp_amd.tiled import GMAX, LMAX, SEG, _tile_count_words, build_tiles, tile_row_counts

# rpt_max, cap and nt are what ``PdlpEngine.tile_limits`` reports for a handle of that precision.  ``group`` -- the items one
# register group of pass 1 holds -- is not reported by the library: it is nt * 4 * TileCfg<T, TV>::TU (TU = 4 for <float, float>,
# 2 for <double, double> and <double, float>; TGRP in k_tiled_fused)
Limits = namedtuple("Limits", "rpt_max cap group nt")
LIMITS = {"f32": Limits(40, 16384, 8192, 512), "f64": Limits(24, 8192, 4096, 512), "mixed": Limits(40, 16384, 4096, 512)}
VALUE_DTYPE = {"f32": torch.float32, "f64": torch.float64, "mixed": torch.float32}      # of the matrix (mixed: float32 under float64 vectors)
UNIT = {"f32": 2.0 ** -24, "f64": 2.0 ** -53, "mixed": 2.0 ** -53}                       # of the vectors, products and row sums
TINY = {"f32": float(np.finfo(np.float32).tiny), "f64": float(np.finfo(np.float64).tiny), "mixed": float(np.finfo(np.float64).tiny)}
NAMES = ("cap_and_groups", "counts", "word4", "empties", "ragged_1x1", "ragged", "remainder", "many_groups", "remainder_tails")
GROUPS = dict(cap_and_groups=(1, 2, 3), empties=(1, 2, 3, 5), many_groups=(1, 4, 5, 8, 9))      # panel groups a case runs with (others: 1)
FUSED_AGAINST_GROUPS = ("cap_and_groups", "empties", "many_groups")       # group counts compared with the one-launch product


@dataclass
class Case:
    name: str
    A: sp.csr_matrix                   # float64 whose every value is a float32 number
    args: dict                         # build_tiles: lw, rpt and, where not the default, max_rest
    groups: tuple = (1,)
    predicates: list = field(default_factory=list)     # (what, function of the built Tiles -> bool)
    other_side_csr: bool = False       # the transpose cannot be tiled with ``args``: that side stays on the CSR kernel


def _f32(v):
    return np.asarray(v, np.float32).astype(np.float64)


def matrix_from_counts(cnt, lw, ncols, seed):
    """CSR with ``cnt[row, panel]`` entries of ``row`` in panel ``panel``: entry j of k sits at a random place of the j-th of k
    equal strata of the panel (distinct and ascending by construction, for any k up to the panel's width)"""
    rng = np.random.default_rng(seed)
    cnt = np.asarray(cnt, np.int64)
    m, P = cnt.shape
    W = 1 << lw
    assert P == max(1, -(-ncols // W))
    width = np.minimum(W, ncols - np.arange(P) * W)
    assert (cnt >= 0).all() and (cnt <= width[None, :]).all()
    k = cnt.reshape(-1)
    total = int(k.sum())
    cell = np.repeat(np.arange(m * P), k)
    j = np.arange(total) - np.repeat(np.cumsum(k) - k, k)
    kk, w, panel = k[cell], width[cell % P], cell % P
    lo, hi = j * w // kk, (j + 1) * w // kk
    col = panel * W + lo + np.minimum((rng.random(total) * (hi - lo)).astype(np.int64), hi - lo - 1)
    indptr = np.concatenate([[0], np.cumsum(cnt.sum(1))])
    val = _f32(rng.standard_normal(total))
    val[val == 0] = 1.0
    A = sp.csr_matrix((val, col.astype(np.int32), indptr.astype(np.int64)), shape=(m, ncols))
    assert np.all(np.diff(col)[np.diff(cell // P) == 0] > 0)               # ascending and distinct inside every row
    return A


def _spread(total, rows, rng):
    """``total`` items over ``rows`` rows as evenly as whole numbers allow"""
    out = np.full(rows, total // rows, np.int64)
    out[rng.choice(rows, total % rows, replace=False)] += 1
    return out


# ---- what the predicates look at ---------------------------------------------------------------------------------------
def counts(t):
    """[tile][row of the row block] items, from the count nibbles the kernel reads"""
    if getattr(t, "_edge_counts", (None,))[0] != t.cnt.data_ptr():          # (unpacked once per count array; read only)
        t._edge_counts = (t.cnt.data_ptr(), torch.stack([tile_row_counts(t, k) for k in range(t.nblk * t.npanel)]).cpu().numpy())
    return t._edge_counts[1]


def runs(t, c=None):
    """[tile][wave][i] items of the 64 consecutive rows that one i of one wave covers"""
    c = counts(t) if c is None else c
    return c.reshape(c.shape[0], t.nt // 64, t.rpt, 64).sum(-1)


def real_sizes(t, c=None):
    return (counts(t) if c is None else c).sum(1)


def padded_sizes(t):
    return np.diff(t.tile_ptr.cpu().numpy())


def words(t, tile):
    """[thread][word] count words of one tile as unsigned numbers"""
    return _tile_count_words(t, tile).cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def format_violations(t, lim):
    """what the kernel trusts and never checks: the list is empty for a tile set that may be attached"""
    c = counts(t)
    bad = []
    if c.max(initial=0) > LMAX:
        bad.append(f"a row holds {c.max()} items of one tile (4-bit counts: at most {LMAX})")
    if runs(t, c).max(initial=0) > GMAX:
        bad.append(f"64 consecutive rows hold {runs(t, c).max()} items of one tile (8-bit scan fields: at most {GMAX})")
    if max(padded_sizes(t).max(initial=0), c.sum(1).max(initial=0)) > lim.cap or t.cap > lim.cap:
        bad.append(f"a tile holds {padded_sizes(t).max()} items (at most {lim.cap})")
    if t.rpt > lim.rpt_max or t.rpt_max != lim.rpt_max or t.nt != lim.nt:
        bad.append(f"built for rpt_max {t.rpt_max}, nt {t.nt}")
    if t.nrem and int(np.diff(t.rem_sptr.cpu().numpy()).max()) > SEG:
        bad.append("a remainder segment is longer than 512 items")
    return bad


# ---- the cases -------------------------------------------------------------------------------------------------------
def cap_and_groups(lim):
    """A: one tile of exactly ``cap`` items, one of exactly one register group, one of a register group and one item; a ragged
    second row block"""
    rng = np.random.default_rng(101)
    lw, rpt = 6, lim.rpt_max
    RB = lim.nt * rpt
    m, n = RB + 100, 150                                       # panels of 64, 64 and 22 columns
    cnt = np.zeros((m, 3), np.int64)
    for p, size in enumerate((lim.cap, lim.group, lim.group + 1)):
        cnt[:RB, p] = _spread(size, RB, rng)
    cnt[RB:, :] = 2
    pads = lambda t: padded_sizes(t)
    return Case("cap_and_groups", matrix_from_counts(cnt, lw, n, 1), dict(lw=lw, rpt=rpt), (1, 2, 3), [
        ("two row blocks by three panels", lambda t: (t.nblk, t.npanel) == (2, 3)),
        ("tile (0, 0) holds exactly cap items", lambda t: real_sizes(t)[0] == lim.cap == pads(t)[0]),
        ("tile (0, 1) holds exactly one register group", lambda t: real_sizes(t)[1] == lim.group == pads(t)[1]),
        ("tile (0, 2) holds one item more than a register group", lambda t: real_sizes(t)[2] == lim.group + 1 and pads(t)[2] == lim.group + 256),
        ("the ragged block has 2 items per row and tile", lambda t: real_sizes(t)[3:].tolist() == [200, 200, 200]),
        ("padded sizes are multiples of 256", lambda t: bool(np.all(pads(t) % 256 == 0))),
        ("no remainder", lambda t: t.nrem == 0),
    ])


def counts_case(lim):
    """B: 64-row runs of exactly 255 items in all eight fields of count word 0 at once (and in word 1), counts 4, 5 and 15"""
    lw, rpt, nt = 6, 9, lim.nt
    RB, nw = nt * rpt, nt // 64
    pat = [15, 0, 5, 4, 1, 15, 0, 0, 3, 2]
    full = min(nw - 1, (lim.cap - 2 * sum(pat)) // (GMAX * rpt))          # waves whose every run holds 255 items of panel 0
    c = np.zeros((nw, rpt, 64), np.int64)                                  # [wave][i][lane]: row = wave*64*rpt + i*64 + lane
    for w in range(full):
        for i in range(rpt):
            c[w, i, :] = 4
            c[w, i, (w * rpt + i) % 64] = 3
    c[full, 0, :10] = pat
    c[full, rpt - 1, 54:] = pat
    cnt = np.zeros((RB, 2), np.int64)
    cnt[:, 0] = c.reshape(-1)
    waves1 = min(nw, lim.cap // (20 * (64 * rpt // 7 + 1)))                 # panel 1: as many waves of rows as cap allows
    r = np.arange(waves1 * 64 * rpt)
    cnt[r[r % 7 == 0], 1] = 15
    cnt[r[r % 7 == 3], 1] = 5

    def followed(t):
        q = runs(t)[0].reshape(-1)
        return bool(np.any((q[:-1] == GMAX) & (q[1:] > 0)))

    return Case("counts", matrix_from_counts(cnt, lw, 128, 2), dict(lw=lw, rpt=rpt), (1,), [
        ("one row block by two panels", lambda t: (t.nblk, t.npanel) == (1, 2)),
        ("the largest 64-row total is 255", lambda t: runs(t).max() == GMAX),
        ("all eight fields of word 0 are full at once, word 1 is in use", lambda t: bool(np.all(runs(t)[0, 0, :8] == GMAX)) and runs(t)[0, 0, 8] == GMAX),
        ("that holds for every wave cap allows", lambda t: full >= 3 and bool(np.all(runs(t)[0, :full] == GMAX))),
        ("the largest count is 15", lambda t: counts(t).max() == LMAX),
        ("counts 4, 5 and 15 are all present, 5 and 15 in both tiles",
         lambda t: {4, 5, 15} <= set(np.unique(counts(t)[0]).tolist()) and {5, 15} <= set(np.unique(counts(t)[1]).tolist())),
        ("a run of 255 is directly followed by a non-empty run", followed),
        ("no tile is above cap, none is in the remainder", lambda t: real_sizes(t).max() <= lim.cap and t.nrem == 0),
    ])


def word4(lim):
    """C: counts only in rows i >= 32, i.e. in count word 4 -- the word-major array behind the [tile][thread][4] entries -- and
    no two of those words equal.  The float64 kernel has three words per thread: rows i >= 16 (word 2) instead"""
    rng = np.random.default_rng(103)
    high = lim.rpt_max // 8 > 4
    rpt, i0, base = (37, 32, 6) if high else (24, 16, 4)
    nd, word, nt = rpt - i0, i0 // 8, lim.nt
    RB, nw, P = nt * rpt, nt // 64, 2
    m = 2 * RB - 700
    code = 1 + rng.permutation(base ** nd - 1)[:2 * P * nt]                 # distinct, none all-zero
    digit = (code[:, None] // base ** np.arange(nd)[None, :]) % base        # [tile*thread][i - i0]
    c = np.zeros((2, P, nw, rpt, 64), np.int64)                             # [block][panel][wave][i][lane]
    c[:, :, :, i0:, :] = digit.reshape(2, P, nw, 64, nd).transpose(0, 1, 2, 4, 3)
    sprinkled = np.zeros((2, P, nw, 64), bool)                              # threads that also carry an item in a row i < i0
    for _ in range(300):
        b, p, w, i, l = (int(rng.integers(k)) for k in (2, P, nw, i0, 64))
        c[b, p, w, i, l] = 1
        sprinkled[b, p, w, l] = True
    cnt = c.transpose(0, 2, 3, 4, 1).reshape(2 * RB, P)[:m]
    sprinkled = sprinkled.reshape(2 * P, nt)

    def high_words(t):
        return np.stack([words(t, k)[:, word] for k in range(4)])

    def low_words_zero(t):
        return all(bool(np.all(words(t, k)[~sprinkled[k], :word] == 0)) and bool(np.any(words(t, k)[sprinkled[k], :word] != 0)) for k in range(4))

    def distinct(t):
        w = high_words(t)
        w = w[w != 0]
        return w.size >= 4 * nt - 2 * 64 and np.unique(w).size == w.size    # (the last wave of the ragged block has no rows i >= i0)

    return Case("word4", matrix_from_counts(cnt, 6, 128, 3), dict(lw=6, rpt=rpt), (1,), [
        ("two row blocks by two panels", lambda t: (t.nblk, t.npanel, t.cw) == (2, 2, word + 1)),
        (f"count word {word} is non-zero in all four tiles", lambda t: bool(np.all((high_words(t) != 0).sum(1) >= nt - 64))),
        (f"words 0..{word - 1} are zero for the threads that carry only rows i >= {i0}", low_words_zero),
        (f"no two count words {word} are equal", distinct),
        ("nothing in the remainder", lambda t: t.nrem == 0),
    ])


def empties(lim):
    """D: empty tiles first, last and in the middle of a row block, and a row block with one non-empty row"""
    rng = np.random.default_rng(104)
    rpt = 2
    RB = lim.nt * rpt
    m, n = 3 * RB, 300                                          # 5 panels, the last one 44 columns wide
    cnt = rng.integers(0, 4, (m, 5))
    cnt[:RB, 0] = 0
    cnt[:RB, 4] = 0
    cnt[RB:2 * RB, 1:3] = 0
    cnt[2 * RB:, :] = 0
    cnt[m - 1, :] = 2
    empty = [0, 4, 5 + 1, 5 + 2]

    def last_block(t):
        c = counts(t)[10:]
        return bool(np.all(c[:, RB - 1] == 2)) and c.sum() == 10

    return Case("empties", matrix_from_counts(cnt, 6, n, 4), dict(lw=6, rpt=rpt), (1, 2, 3, 5), [
        ("three row blocks by five panels", lambda t: (t.nblk, t.npanel) == (3, 5)),
        ("tiles (0,0), (0,4), (1,1) and (1,2) are empty", lambda t: all(real_sizes(t)[k] == 0 == padded_sizes(t)[k] for k in empty)),
        ("every other tile of blocks 0 and 1 is not", lambda t: all(real_sizes(t)[k] > 0 for k in range(10) if k not in empty)),
        ("block 2 holds its last row only", last_block),
        # group g of n walks the panels [5g/n, 5(g+1)/n): with 3 groups, group 1 owns panels 1 and 2 -- both empty in block 1
        ("with 3 groups one group of block 1 owns only empty panels", lambda t: [t.npanel * 1 // 3, t.npanel * 2 // 3] == [1, 3]),
    ])


def ragged_1x1(lim):
    A = sp.csr_matrix(np.array([[1.5]]))
    return Case("ragged_1x1", A, dict(lw=6, rpt=1), (1,), [
        ("one tile of one item", lambda t: (t.nblk, t.npanel, t.items) == (1, 1, 256) and real_sizes(t).tolist() == [1]),
    ])


def ragged(lim):
    """E (b): one row and one column more than whole tiles; entries on the first and last column of every panel.  Its
    transpose has 193 rows of about 2900 entries: nearly all of them would leave the tiles, so that side stays on the CSR kernel"""
    rng = np.random.default_rng(105)
    rpt, W = 7, 64
    m, n = lim.nt * rpt + 1, 3 * W + 1
    rows = np.array([r for r in range(m) if r % 5 != 2 or r == m - 1])
    cols = np.array([0, W - 1, W, 2 * W - 1, 2 * W, 3 * W - 1, 3 * W])
    rr, cc = np.repeat(rows, cols.size), np.tile(cols, rows.size)
    A = sp.csr_matrix((_f32(rng.standard_normal(rr.size)), (rr, cc)), shape=(m, n))
    A.sort_indices()
    return Case("ragged", A, dict(lw=6, rpt=rpt), (1,), [
        ("two row blocks by four panels", lambda t: (t.nblk, t.npanel) == (2, 4)),
        ("the second block holds the last row only: 2, 2, 2 and 1 items", lambda t: real_sizes(t)[4:].tolist() == [2, 2, 2, 1]),
        ("every fifth row is empty", lambda t: bool(np.all(counts(t)[:4].reshape(4, -1)[:, 2::5] == 0))),
        ("the last panel is one column wide", lambda t: t.ncols - (t.npanel - 1) * W == 1),
    ], other_side_csr=True)


def _long_rows(m, n, lengths, seed, others=3):
    cnt = np.full((m, 1), others, np.int64)
    for r, k in lengths.items():
        cnt[r, 0] = k
    return matrix_from_counts(cnt, 16, n, seed)


def remainder(lim):
    """F: rows of more than 15 items in one panel: remainder segments of 512, 1 and 7 items, a row of 65 segments"""
    A = _long_rows(3000, 40000, {5: 15 + 512, 6: 15 + 513, 700: 15 + 64 * 512 + 7, 2999: 16}, 6)
    seg = lambda t: np.diff(t.rem_sptr.cpu().numpy())
    return Case("remainder", A, dict(lw=16, rpt=3, max_rest=0.95), (1,), [
        ("remainder rows 5, 6, 700 and 2999", lambda t: t.rem_rows.tolist() == [5, 6, 700, 2999]),
        ("of 1, 2, 65 and 1 segments", lambda t: np.diff(t.rem_rptr.cpu().numpy()).tolist() == [1, 2, 65, 1]),
        ("segments of 512, 1 and 7 items", lambda t: {512, 1, 7} <= set(seg(t).tolist()) and seg(t).max() == 512),
        ("15 items of those rows stay in the tiles", lambda t: t.nrem == 512 + 513 + 64 * 512 + 7 + 1),
    ])


def remainder_tails(lim):
    """H (added for mutants 5, 6 and 7): k_rem_segments and k_rem_rows load eight clamped entries per lane and round trip, and the
    clamped copy of the last one lands on a lane only when the count is 8 or more past a multiple of 64 -- segments of 20, 100, 8,
    63 and 71 items, a row of 9 segments.  Remainder rows at i = 0, 1, 5, 8, 9 and 11 of their threads: the fused epilogue adds
    the remainder's sums in groups of 8 (4) rows per thread"""
    rpt = 12
    rows = {10: 15 + 20, 64 * 5 + 1: 15 + 100, 64 * 9 + 2: 15 + 8, 64 * 11 + 63: 15 + 63, lim.nt * rpt + 64 * 8: 15 + 8 * 512 + 5, 6999: 15 + 71}
    A = _long_rows(7000, 40000, rows, 8, others=1)               # (6144 rows per tile: below the float64 cap)
    seg = lambda t: np.diff(t.rem_sptr.cpu().numpy())
    i_of = lambda t: sorted(set(((r % (t.nt * rpt)) % (64 * rpt)) // 64 for r in t.rem_rows.tolist()))
    return Case("remainder_tails", A, dict(lw=16, rpt=rpt, max_rest=0.95), (1,), [
        ("remainder rows", lambda t: t.rem_rows.tolist() == sorted(rows)),
        ("segments whose length is 8 or more past a multiple of 64", lambda t: {20, 100, 8, 63, 71} <= set(seg(t).tolist())),
        ("a row of 9 segments", lambda t: np.diff(t.rem_rptr.cpu().numpy()).tolist() == [1, 1, 1, 1, 9, 1]),
        ("remainder rows in the thread's rows 0..3, 4..7 and 8..11", lambda t: i_of(t) == [0, 1, 5, 8, 9, 11]),
    ])


def many_groups(lim):
    """G: 9 panels in 4, 5, 8 and 9 groups: k_rowsum_epilogue adds the partial sums four groups at a time.  ``build_tiles`` folds
    4 groups of 9 panels to 3 and 8 to 5 (``normalize_groups``); the library takes any count up to the number of panels and the
    kernel gives group g of n the panels [9g/n, 9(g+1)/n), so ``with_groups`` sets the field the ABI carries"""
    rng = np.random.default_rng(107)
    m, n = 600, 9 * 64
    cnt = rng.integers(0, 4, (m, 9))
    cnt[17, :] = 0
    cnt[599, :] = [15, 0, 1, 0, 0, 2, 0, 0, 5]
    return Case("many_groups", matrix_from_counts(cnt, 6, n, 7), dict(lw=6, rpt=1), (1, 4, 5, 8, 9), [
        ("two row blocks by nine panels", lambda t: (t.nblk, t.npanel) == (2, 9)),
        ("no tile is empty", lambda t: real_sizes(t).min() > 0),
    ])


_MAKERS = dict(cap_and_groups=cap_and_groups, counts=counts_case, word4=word4, empties=empties, ragged_1x1=ragged_1x1, ragged=ragged,
               remainder=remainder, many_groups=many_groups, remainder_tails=remainder_tails)
_CASES = {}


def get_case(name, prec):
    """built once per session, shared, never written to"""
    key = (name, LIMITS[prec])
    if key not in _CASES:
        _CASES[key] = _MAKERS[name](LIMITS[prec])
        assert _CASES[key].groups == GROUPS.get(name, (1,))
    return _CASES[key]


def params():
    """(case, precision, side, groups) of every GPU test"""
    return [(n, p, s, g) for n in NAMES for p in LIMITS for s in ("K", "KT") for g in GROUPS.get(n, (1,))]


# ---- building -----------------------------------------------------------------------------------------------------------
def with_groups(t, groups):
    """the tile set with ``groups`` panel groups.  ``build_tiles`` has folded counts that leave ceil(P/groups)-panel groups empty;
    the kernel splits the panels evenly and the library accepts any count up to the number of panels"""
    assert 1 <= groups <= t.npanel
    t.groups = int(groups)
    return t


def build(case, prec, groups=1, transposed=False, device="cpu", max_groups=32):
    """Tiles of the case matrix (or of its transpose, with the same explicit arguments), or None where it cannot be tiled"""
    lim = LIMITS[prec]
    A = case.A.T.tocsr() if transposed else case.A
    A.sort_indices()
    dev = lambda v, dt: torch.tensor(np.asarray(v), dtype=dt, device=device)
    t = build_tiles(dev(A.indptr, torch.int32), dev(A.indices, torch.int32), dev(A.data, VALUE_DTYPE[prec]), A.shape[0], A.shape[1],
                    groups=groups, max_groups=max_groups, kernel_limits=(lim.rpt_max, lim.cap, lim.nt), **case.args)
    return None if t is None else with_groups(t, groups)


# ---- the reference of the product ---------------------------------------------------------------------------------------
def probe(n, seed=5):
    """a vector of float32 numbers: every product with a float32 matrix value is exact in float64"""
    return _f32(np.random.default_rng(3000 + seed).standard_normal(n))


def exact_product(A, v):
    """(correctly rounded row sums of the exact products, sum_j |K_ij| |v_j|, items per row): ``math.fsum``, no kernel has a part in it"""
    A = sp.csr_matrix(A)
    prod = A.data * v[A.indices]
    assert np.array_equal(prod.astype(np.float64), prod) and A.data.dtype == np.float64
    ip = A.indptr
    items = np.diff(ip)
    ref = np.zeros(A.shape[0])
    ref[items == 1] = prod[ip[:-1][items == 1]]            # (rows of one item: the exact product itself; of none: 0)
    mag = np.abs(ref)
    for r in np.flatnonzero(items > 1):
        ref[r] = math.fsum(prod[ip[r]:ip[r + 1]])
        mag[r] = math.fsum(np.abs(prod[ip[r]:ip[r + 1]]))
    return ref, mag, items


def product_bound(prec, mag, items):
    """|row sum - exact| <= (L + 1) u sum_j |K_ij| |v_j| + the smallest normal number: L roundings of products and additions in any
    order on an item's way into its row sum, one more for the remainder's sum joining the tiles' (as in tests/test_gpu_report.py);
    with u = 2^-53 the reference's own rounding, at most u |ref|, stays inside because the products themselves are exact there"""
    return (items + 1) * UNIT[prec] * mag + TINY[prec]


# ---- the LP around a case matrix (the epilogue check) -------------------------------------------------------------------------
SEQUENCE = [("set_iterate", 1), ("set_step", 1.0, 1.25, 0), ("iterate", 1, False), ("kkt", "CUR", 1.25, False), ("iterate", 1, True),
            ("kkt", "CUR", 1.25, False), ("report", "CUR", False, 1.0), ("detect_infeasibility", 1e-3)]
_LPS = {}


def get_lp(name, prec, side):
    """HostLP whose K (side "K") or K' (side "KT") is the case matrix: all four bound classes, m_ineq = 2m/5 as ``sparse_lp``"""
    from tests.host_lp import HostLP, _bounds
    key = (name, LIMITS[prec], side)
    if key not in _LPS:
        A = get_case(name, prec).A
        A = A.T.tocsr() if side == "KT" else A
        m, n = A.shape
        rng = np.random.default_rng(900 + NAMES.index(name))
        l, u = _bounds(rng, n, True)
        _LPS[key] = HostLP(A, (2 * m) // 5, rng.standard_normal(n), rng.standard_normal(m), l, u)
    return _LPS[key]
