"""7-byte items on the GPU: the device packer against its CPU model byte for byte, and every result of a float32 engine bit for
bit the same from the packed index stream (PDLP_PACKED_ITEMS=1) as from the 32-bit words (=0) -- plain products with K and K',
five adaptive iterations, fused launches and panel groups, a matrix with a remainder.  A tile set that does not qualify stays on
the 32-bit words, and so does a mixed-precision engine.

Shapes: the smallest at which tiles are dense enough to qualify.  A tile may hold 255 items of 64 consecutive rows, i.e. under
four per row and panel, so the matrices have three items per row and panel and row blocks of 5120 rows (about 15 000 items per
tile, a run of 64 spans some 300 columns): 43 520 x 65 536 with 3 per row (one 64K panel, nine row blocks, the last one half
full -- a last block of a few rows would be a sparse tile and the matrix would not qualify), 43 520 x 131 072 with 6 (two panels),
30 000 x 20 000 with 14 (``choose_lw`` narrows the panels to
4096 columns: five panels)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import torchpdlp_amd as tp
from torchpdlp_amd import _native as N
from torchpdlp_amd import tiled as T

DEV = torch.device("cuda", 0)
CASES = {"one_panel": (43_520, 65_536, 3), "two_panels": (43_520, 131_072, 6), "narrow_panels": (30_000, 20_000, 14)}
_LP = {}


def _lp(name, dense_row=False):
    """the LP of a case on the device (made once, never written to); ``dense_row``: row 7 of K holds 5000 items -- more than 15 per
    tile -- so K gets a remainder, and K' has 5000 rows that meet it"""
    key = (name, dense_row)
    if key not in _LP:
        m, n, k = CASES[name]
        lp = tp.gen_lp(n, m, k, seed=11, device="cpu")                  # (columns, rows, items per row)
        assert (lp.m, lp.n) == (m, n)
        rp, ci, va = lp.rowptr.long(), lp.colidx, lp.val
        if dense_row:
            g = torch.Generator().manual_seed(5)
            cols = torch.randperm(n, generator=g)[:5000].sort().values.to(ci.dtype)
            a, b = int(rp[7]), int(rp[8])
            ci = torch.cat([ci[:a], cols, ci[b:]])
            va = torch.cat([va[:a], torch.randn(5000, generator=g).to(va.dtype), va[b:]])
            rp = rp.clone()
            rp[8:] += 5000 - (b - a)
        K = tp.CsrPair(m, n, rp.to(lp.rowptr.dtype), ci, va).to(DEV)
        _LP[key] = (K, tuple(t.to(DEV) for t in (lp.c, lp.q, lp.l, lp.u)), lp.m_ineq)
    return _LP[key]


def _engine(monkeypatch, name, packed, groups=None, dense_row=False, **kw):
    monkeypatch.setenv("PDLP_TILED", "1")
    monkeypatch.setenv("PDLP_TILE_RPT", "10")          # 5120-row blocks (the builder's own choice for so few rows: 512-row blocks, sparse tiles)
    if packed is None:
        monkeypatch.delenv("PDLP_PACKED_ITEMS", raising=False)
    else:
        monkeypatch.setenv("PDLP_PACKED_ITEMS", packed)
    if groups is not None:
        monkeypatch.setenv("PDLP_TILE_GROUPS", str(groups))
    K, (c, q, l, u), m_ineq = _lp(name, dense_row)
    if kw.get("vec_dtype") is torch.float64:
        c, q, l, u = (t.double() for t in (c, q, l, u))
    eng = tp.PdlpEngine.from_full(K, c, q, l, u, m_ineq, **kw)
    assert all(t is not None for t in eng.tiles), eng.kernels
    return eng


def _results(eng):
    """plain products with K and K', then five adaptive iterations: everything as bytes on the host"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(eng.n, generator=g).to(eng.dtype).to(DEV)
    y = torch.randn(eng.m, generator=g).to(eng.dtype).to(DEV)
    out = {"Kx": eng.spmv(x, False), "KTy": eng.spmv(y, True)}
    eng.set_iterate(torch.zeros(eng.n, dtype=eng.dtype, device=DEV), torch.zeros(eng.m, dtype=eng.dtype, device=DEV))
    eng.set_step(0.05, 1.0, 1.0, 0)
    eng.iterate(5, True)
    out["x"], out["y"] = eng.get_iterate(N.CUR)
    s = eng.scalars()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["eta"], out["omega"] = np.float64(s["eta"]), np.float64(s["omega"])
    return out


def _same(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{k} differs between the 32-bit and the packed index stream"
    assert np.all(np.isfinite(a["x"])) and np.all(np.isfinite(a["y"])) and np.any(a["x"] != 0) and np.any(a["Kx"] != 0)


@pytest.mark.parametrize("name", list(CASES))
def test_device_packer_matches_the_model(monkeypatch, name):
    eng = _engine(monkeypatch, name, "1")
    for tr in (0, 1):
        t = eng.tiles[tr]
        assert t.stats["packed_items"] is True and "32-bit items" not in eng.kernels[tr]
        assert 7.0 < t.stats["bytes_per_nnz"] < (t.items * 8 + t.cnt.numel() * 4) / t.stats["tiled"]
        host = T.Tiles(t.lw, t.rpt, t.cap, t.nblk, t.npanel, t.nrows, t.ncols, t.idx.cpu(), t.val.cpu(), t.tile_ptr.cpu(), t.cnt.cpu(),
                       t.groups, t.rpt_max, t.nt)
        idx24, run_base, fits = T.pack_items24(host)
        assert fits
        assert torch.equal(t._idx24.cpu(), idx24) and torch.equal(t._run_base.cpu(), run_base)
        assert torch.equal(T.unpack_items24(t._idx24.cpu(), t._run_base.cpu(), host), host.idx)


@pytest.mark.parametrize("name,groups,dense_row", [("one_panel", None, False), ("two_panels", None, False), ("narrow_panels", None, False),
                                                    ("two_panels", 2, False), ("narrow_panels", 2, False), ("one_panel", None, True),
                                                    ("narrow_panels", 2, True)])
def test_packed_and_32bit_streams_give_the_same_bits(monkeypatch, name, groups, dense_row):
    e0 = _engine(monkeypatch, name, "0", groups, dense_row)
    r0 = _results(e0)
    assert not any(t.stats["packed_items"] for t in e0.tiles) and all(k.endswith(", 32-bit items") for k in e0.kernels), e0.kernels
    e1 = _engine(monkeypatch, name, "1", groups, dense_row)
    assert all(t.stats["packed_items"] for t in e1.tiles) and not any("32-bit items" in k for k in e1.kernels), e1.kernels
    if groups:
        assert e1.tiles[0].groups == groups and f"tiled/{groups} groups" in e1.kernels[0], e1.kernels      # (K' of two_panels has one panel)
    else:
        assert all(t.groups == 1 for t in e1.tiles)
    if dense_row:
        assert e1.tiles[0].nrem >= 5000 - 15 * e1.tiles[0].npanel and "remainder" in e1.kernels[0]
    _same(r0, _results(e1))
    # and back: detaching the packed stream leaves the 32-bit launches
    for tr in (0, 1):
        N.check(e1.lib.pdlp_attach_packed_items(e1.h, tr, None, None))
    _same(r0, _results(e1))


def test_a_tile_set_that_does_not_qualify_stays_on_the_32bit_words(monkeypatch):
    """2000 x 200 000 with 3 per row: about 1500 items per 64K-column tile, a run of 64 spans some 2800 columns"""
    monkeypatch.setenv("PDLP_TILED", "1")
    monkeypatch.setenv("PDLP_TILE_LW", "16")
    lp = tp.gen_lp(200_000, 2000, 3, seed=2, device="cpu")
    K = tp.CsrPair(lp.m, lp.n, lp.rowptr, lp.colidx, lp.val).to(DEV)
    vec = tuple(t.to(DEV) for t in (lp.c, lp.q, lp.l, lp.u))
    res = {}
    for mode in ("0", "auto"):
        monkeypatch.setenv("PDLP_PACKED_ITEMS", mode)
        monkeypatch.setattr("torchpdlp_amd.engine_kernels.PACKED_ITEMS_DEFAULT", True)          # whatever the shipped default is
        eng = tp.PdlpEngine.from_full(K, *vec, lp.m_ineq)
        assert eng.tiles[0] is not None and eng.tiles[0].stats["packed_items"] is False
        assert eng.kernels[0].startswith("tiled") and eng.kernels[0].endswith(", 32-bit items")          # it says so
        res[mode] = _results(eng)
    _same(res["0"], res["auto"])
    monkeypatch.setenv("PDLP_PACKED_ITEMS", "1")
    with pytest.raises(N.PdlpError, match="1023 columns"):
        tp.PdlpEngine.from_full(K, *vec, lp.m_ineq)


def test_mixed_precision_keeps_the_32bit_words(monkeypatch):
    """float32 tiles under float64 vectors read the 32-bit words whatever the variable says"""
    res = {}
    for mode in (None, "0", "1"):
        eng = _engine(monkeypatch, "one_panel", mode, vec_dtype=torch.float64, delta=False)
        assert eng.mixed and not any(t.stats["packed_items"] for t in eng.tiles) and not any("items" in k for k in eng.kernels)
        t = eng.tiles[0]
        # the library refuses the packed stream on such a handle
        dummy = torch.zeros(64, dtype=torch.int32, device=DEV)
        assert eng.lib.pdlp_attach_packed_items(eng.h, 0, dummy.data_ptr(), dummy.data_ptr()) == -3
        res[mode] = _results(eng)
    _same(res[None], res["0"])
    _same(res[None], res["1"])
