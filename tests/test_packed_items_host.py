"""7-byte items on the CPU: the packed index stream of a float32 tile set (``pack_items24`` / ``unpack_items24`` in
torchpdlp_amd/tiled.py, the model of the device packer) reproduces the 32-bit index words exactly, and the eligibility rule."""
import numpy as np
import pytest
import torch

from torchpdlp_amd import tiled as T
from torchpdlp_amd.tiled import build_tiles, choose_lw, pack_items24, packed_items_shape_ok, unpack_items24


def _csr(m, n, lens, seed):
    rng = np.random.default_rng(seed)
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    ci = np.concatenate([np.sort(rng.choice(n, size=int(k), replace=False)) for k in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    va = rng.standard_normal(int(rp[-1])).astype(np.float32)
    return torch.from_numpy(rp.astype(np.int32)), torch.from_numpy(ci), torch.from_numpy(va)


def _roundtrip(t):
    idx24, run_base, fits = pack_items24(t)
    assert fits
    assert idx24.dtype == torch.int32 and idx24.numel() * 4 == 3 * t.items                  # 3 bytes per stored item
    assert run_base.numel() == 2 * (t.items // 256 + T.P24_TAIL) and not bool(run_base[2 * (t.items // 256):].any())
    assert np.all(3 * t.tile_ptr.numpy() % 768 == 0)                                        # byte offset of a tile = 3 x its item offset
    assert torch.equal(unpack_items24(idx24, run_base, t), t.idx)
    return idx24, run_base


def _dense_case(m, n, per_row, lw, seed=3, **kw):
    rp, ci, va = _csr(m, n, np.full(m, per_row), seed)
    t = build_tiles(rp, ci, va, m, n, lw=lw, **kw)
    assert t is not None
    return t


def test_roundtrip_lw16_small_random():
    """65536-column panels (the bench's width) over a small matrix: one panel, two row blocks with a short second one, and tiles
    dense enough that a run of 64 sorted items stays inside 1023 columns (three items per row: 64 rows hold at most 255)"""
    m, n = 2200, 3000
    t = _dense_case(m, n, 3, 16, rpt=4)
    assert t.lw == 16 and t.npanel == 1 and t.nblk == 2 and m - t.rows_per_block < t.rows_per_block // 8     # a last row block with few rows
    assert packed_items_shape_ok(t)
    idx24, run_base = _roundtrip(t)
    # a field is (slot << 10) | (column - run base): spot-check the first chunk against the definition
    by = idx24.view(torch.uint8).long().view(-1, 64, 4, 3)
    f = by[..., 0] | (by[..., 1] << 8) | (by[..., 2] << 16)
    w = (t.idx.long() & 0xFFFFFFFF).view(-1, 64, 4)
    rb0 = [int(run_base[0]) & 0xFFFF, (int(run_base[0]) >> 16) & 0xFFFF, int(run_base[1]) & 0xFFFF, (int(run_base[1]) >> 16) & 0xFFFF]
    for j in range(4):
        assert rb0[j] == int((w[0, :, j] & 0xFFFF).min())                                   # (the first chunk of a full tile has no padding)
        assert torch.equal(f[0, :, j], ((w[0, :, j] >> 16) << 10) | ((w[0, :, j] & 0xFFFF) - rb0[j]))


def test_roundtrip_narrow_panels_from_choose_lw():
    """rows so long that ``choose_lw`` narrows the panels: several panels, several tiles per row block"""
    m, n, per_row = 1500, 40_000, 28
    lw = choose_lw(m, m * per_row, n)
    assert lw < 16
    t = _dense_case(m, n, per_row, lw)
    assert t.npanel > 1 and packed_items_shape_ok(t)
    _roundtrip(t)


def test_roundtrip_tile_of_exactly_cap_items_and_empty_tiles():
    """a tile with no padding whose last slot is cap - 1 = 16383 (the largest a 14-bit field holds), next to tiles without items"""
    rpt, m = 40, 512 * 40                                                                   # one full row block of 20480 rows ...
    rng = np.random.default_rng(5)
    rp = torch.clamp(torch.arange(m + 1, dtype=torch.int32), max=16384)                     # ... whose first 16384 rows hold one item each
    ci = torch.from_numpy(rng.integers(1024, 2048, 16384).astype(np.int32))
    va = torch.from_numpy(rng.standard_normal(16384).astype(np.float32))
    t = build_tiles(rp, ci, va, m, 4096, lw=10, rpt=rpt)                                    # panels 0, 2, 3 are empty, panel 1 holds everything
    assert t is not None and t.nrem == 0 and t.cap == 16384
    sizes = np.diff(t.tile_ptr.numpy())
    assert sizes.tolist() == [0, 16384, 0, 0]
    assert int(((t.idx.long() & 0xFFFFFFFF) >> t.lw).max()) == 16383
    _roundtrip(t)
    # and a tile set with no items at all
    e = build_tiles(torch.zeros(11, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0), 10, 300, lw=6, rpt=1)
    assert e is not None and e.items == 0
    idx24, run_base, fits = pack_items24(e)
    assert fits and idx24.numel() == 0 and run_base.numel() == 2 * T.P24_TAIL
    assert unpack_items24(idx24, run_base, e).numel() == 0


def test_padding_keeps_its_slot_and_gets_column_zero():
    t = _dense_case(700, 900, 3, 16, rpt=2)
    idx24, run_base = _roundtrip(t)
    tp = t.tile_ptr.tolist()
    real = T.tile_item_counts(t)
    assert int(real.sum()) == 700 * 3 and any(int(real[k]) % 256 for k in range(len(real)))       # there is padding
    by = idx24.view(torch.uint8).long().view(-1, 64, 4, 3)
    f = (by[..., 0] | (by[..., 1] << 8) | (by[..., 2] << 16)).transpose(1, 2).reshape(-1)    # sorted order inside every chunk
    for k in range(len(real)):
        pad = f[tp[k] + int(real[k]):tp[k + 1]]
        assert bool((pad == (int(real[k]) << 10)).all())                                    # slot = number of real items (<= 16383), column field 0


def test_eligibility():
    # one sparse tile: a run of 64 sorted items spanning more than 1023 columns
    m, n = 600, 60_000
    rp, ci, va = _csr(m, n, np.full(m, 3), 7)
    t = build_tiles(rp, ci, va, m, n, lw=16, rpt=2)
    assert t is not None and packed_items_shape_ok(t)
    assert pack_items24(t)[2] is False
    # the same rows with ONE sparse tile among dense ones: still the whole matrix stays on the 32-bit stream
    lens = np.full(2048 + 200, 3)
    rp, ci, va = _csr(len(lens), 3000, lens, 8)
    ci = ci.clone()
    dense = build_tiles(rp, ci, va, len(lens), 3000, lw=16, rpt=4)
    assert pack_items24(dense)[2] is True
    ci2 = ci.long()
    last = int(rp[2048])                                                                    # the second row block: its columns spread over 64K
    ci2[last:] = ci2[last:] * 21
    wide = build_tiles(rp, ci2.int(), va, len(lens), 65_000, lw=16, rpt=4)
    assert wide is not None and wide.nblk == 2 and pack_items24(wide)[2] is False
    # cap above 16384 (a kernel build with larger tiles), float64 tiles, panels wider than 64K columns
    big = build_tiles(rp, ci, va, len(lens), 3000, lw=12, rpt=4, cap=32768, kernel_limits=(40, 32768, 512))
    assert big is not None and big.cap == 32768 and not packed_items_shape_ok(big)
    f64 = build_tiles(rp, ci, va.double(), len(lens), 3000, lw=12, rpt=4)
    assert f64 is not None and not packed_items_shape_ok(f64)
    w17 = build_tiles(rp, ci, va, len(lens), 3000, lw=17, rpt=4)
    assert w17 is not None and not packed_items_shape_ok(w17)
    with pytest.raises(ValueError):
        pack_items24(w17)
