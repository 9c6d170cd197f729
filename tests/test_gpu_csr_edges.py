"""The CSR kernels (k_csr_fused, its SORTED form and k_long_rows in csrc/pdlp_kernel_csr.inc) on the constructed matrices of
tests/csr_cases.py: every case sits on limits of the kernels' schedule -- blocks of exactly NNZ_CAP items and of ROWS_CAP rows, every
lane count per row, rows of NNZ_CAP + 1 items and of 8, 9 and 17 chunks, blocks without items, more work items than workgroups, a
second workgroup of k_long_rows, sorted blocks 2^21 - 1 and 2^21 columns wide -- in float32, float64 and mixed precision, as K and as
K', in CSR order and with column-sorted row blocks.

Before anything is multiplied, the row blocks the handle holds (``PdlpEngine.schedule_info``) must be the Python model's on both
sides, ``eng.kernels`` must name the form, and under ``sorted`` the count of blocks read sorted must be the model's.

(a) ``test_product``: ``eng.spmv`` with the case matrix and, on the engine's other side, with its transpose, each against the
    per-row ``math.fsum`` of the exact float64 products (matrix and vector hold float32 numbers), within ``(L + 1) u sum_j |K_ij| |v_j|`` plus the smallest normal number, L the row's items, u = 2^-24 (float32) or
    2^-53 (float64, mixed): the bound of any summation order of L rounded products -- the chunk sums that k_long_rows joins are
    additions among the same L - 1.  Rows without items give exactly 0; a second call gives the same bits; the sorted form gives the
    CSR form's product bit for bit (what torchpdlp_amd/tiled.py promises).
(b) ``test_epilogue``: an LP around the case matrix (all four bound classes, m_ineq = 2m/5) and the float64 model of the handle
    (tests/handle_model.py) side by side through ``csr_cases.SEQUENCE`` -- one fixed step at 0.5 / ||K||, a KKT pass, one adaptive
    step, a KKT pass, a report, the detector -- compared after every call at the tolerances of tests/test_gpu_sequences.py: A for
    float64 and mixed, B for float32; after the float32 adaptive step eta within rtol 2e-4.  The model decides that step by a margin
    above 1e-2 (tests/test_csr_cases_host.py).  This is the check that sees the partial sums of long rows and of all-empty blocks
    reach the step-size rule and the KKT sums, and every row without an item get its half-step.
    Nothing is added to B for the long rows: the derived product bound of a row of 34 816 items times the step would allow 0.1 on an
    entry of order 1, the float32 kernel stays inside B's 5e-5 there (the ratios are recorded), so B stands as it is.

The largest error / bound per case, precision, side and form and the file's wall time are printed at the end (``CSR-EDGE-STATS``)
and written to the file ``PDLP_CSR_EDGE_STATS`` names; profiles/r20_csr_edges/ holds a run."""
import json
import os
import re
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as orc                                   # the checker (tests only)
from tests import csr_cases as cc
from tests import tile_cases as tc
from tests.host_lp import DEV
from tests.test_gpu_sequences import A_TOL, B_TOL
from tests.test_gpu_tile_edges import EdgeRun
from torchpdlp_amd import _native as N

PREC = {"f32": (torch.float32, {}, B_TOL), "f64": (torch.float64, {}, A_TOL),
        "mixed": (torch.float32, dict(vec_dtype=torch.float64, delta=False), A_TOL)}
PARAMS = cc.params()
IDS = ["-".join(p) for p in PARAMS]
STATS = {}                           # "case/precision/side/form" -> largest error / bound of each check
_CSR = {}                            # (case, precision, side, transpose) -> the CSR form's product


@pytest.fixture(scope="module", autouse=True)
def _setup():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    orc.set_threads(1)
    N.load()
    t0 = time.time()
    yield
    summary = dict(wall_seconds=round(time.time() - t0, 2), tests=2 * len(PARAMS), worst=STATS)
    print("\nCSR-EDGE-STATS " + json.dumps(summary))
    if os.environ.get("PDLP_CSR_EDGE_STATS"):
        with open(os.environ["PDLP_CSR_EDGE_STATS"], "w") as f:
            json.dump(summary, f, indent=1, sort_keys=True)


def _note(key, what, ratio):
    w = STATS.setdefault("/".join(key), {})
    w[what] = max(w.get(what, 0.0), float(ratio))


def _engine(name, prec, side, form):
    """engine of the LP around the case (side "K": K is the case matrix, "KT": K' is) on the CSR kernel in ``form``, its row blocks
    and its kernel names checked against the model on both sides"""
    assert cc.broken_predicates(name) == [], f"{name} does not hold its edge"
    lp = cc.get_lp(name, side)
    dtype, kw, _ = PREC[prec]
    eng = lp.engine(dtype, form, **kw)
    assert eng.mixed == (prec == "mixed") and not eng.delta and eng.tiles == [None, None]
    for tr in (0, 1):
        of = ("K", "KT")[tr] if side == "K" else ("KT", "K")[tr]
        model = cc.get_sched(name, of)[0]
        got = eng.schedule_info(tr).cpu().numpy()
        assert got.shape == model.blocks.shape and np.array_equal(got, model.blocks), f"{name} {of}: the handle's row blocks are not the model's"
        if form == "csr":
            assert eng.kernels[tr] == "csr"
        else:
            m = re.fullmatch(r"csr, sorted row blocks \((\d+) of (\d+)\)", eng.kernels[tr])
            assert m and (int(m.group(1)), int(m.group(2))) == (cc.n_sorted(name, of), model.nblk), (eng.kernels[tr], cc.n_sorted(name, of), model.nblk)
    return eng, lp


def _product(eng, v, tr):
    """``eng.spmv``, which writes into ``torch.empty``: the block the allocator is about to hand out is filled with NaN first, so a row
    the kernel does not store shows as not finite and never as an earlier product's value.  That the freed block is the one
    ``torch.empty`` gets next is how the caching allocator behaves, not a promise: it holds while ``spmv`` allocates nothing of that
    size before its output (``x`` already has the working type, so ``as_vec`` copies nothing); the epilogue check sees a missing
    store independently"""
    x = torch.tensor(v, dtype=eng.dtype, device=DEV)
    poison = torch.full((eng.nl if tr else eng.ml,), float("nan"), dtype=eng.dtype, device=DEV)
    torch.cuda.synchronize()
    del poison
    return eng.spmv(x, bool(tr)).cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("name,prec,side,form", PARAMS, ids=IDS)
def test_product(name, prec, side, form):
    """both products of the engine: with the case matrix ("product" in the statistics) and with its transpose, the other side of
    the same engine ("product_transposed"), each against its own reference"""
    eng, lp = _engine(name, prec, side, form)
    for tr in (0, 1):
        of = ("K", "KT")[tr] if side == "K" else ("KT", "K")[tr]
        what = "product" if of == "K" else "product_transposed"
        v, ref, mag, items = cc.reference(name, of)
        bound = tc.product_bound(prec, mag, items)
        got = _product(eng, v, tr)
        assert got.shape == ref.shape and np.all(np.isfinite(got)), f"{what}: {int((~np.isfinite(got)).sum())} rows are not finite"
        err = np.abs(got - ref)
        worst = int(np.argmax(err / bound))
        print(f"{what} {name} {prec} {side} {form}: largest error / bound {err[worst] / bound[worst]:.3e} (row {worst}, {items[worst]} items)")
        _note((name, prec, side, form), what, err[worst] / bound[worst])
        assert np.all(err <= bound), f"{what} row {worst}: |{got[worst]!r} - {ref[worst]!r}| = {err[worst]:.3e} > {bound[worst]:.3e}"
        assert np.all(got[items == 0] == 0), f"{what}: a row without items"
        assert np.array_equal(_product(eng, v, tr), got), f"{what} is not deterministic"
        key = (name, prec, side, tr)
        if form == "csr":
            _CSR[key] = got
            continue
        if key not in _CSR:
            _CSR[key] = _product(_engine(name, prec, side, "csr")[0], v, tr)
        differ = np.flatnonzero(_CSR[key] != got)
        assert differ.size == 0, f"{what}: {differ.size} rows differ from the CSR form's, the first: row {differ[0]}, {got[differ[0]]!r} != {_CSR[key][differ[0]]!r}"


class CsrEdgeRun(EdgeRun):
    """tests/test_gpu_tile_edges.py's comparison of an engine with the model, call by call; the ratios go to this file's STATS"""

    def note(self, what, dev, bound):
        assert np.isfinite(dev), self.message(what)
        if bound > 0:
            _note(self.key, "epilogue", dev / bound)
        assert dev <= bound, self.message(f"{what}: |engine - model| = {dev:.3e} > {bound:.3e}")


@pytest.mark.parametrize("name,prec,side,form", PARAMS, ids=IDS)
def test_epilogue(name, prec, side, form):
    eng, lp = _engine(name, prec, side, form)
    cfg = f"{name}-{prec}-{side}-{form}"
    run = CsrEdgeRun((name, prec, side, form), prec, cfg, lp, eng, PREC[prec][2])
    run.run(cfg, cc.SEQUENCE)
    assert run.adaptive_done and eng.scalars()["k"] == 2
    print(f"epilogue {cfg}: largest deviation / tolerance {STATS['/'.join(run.key)]['epilogue']:.3e}")
