"""The panel-tiled kernel (k_tiled_fused with k_rowsum_epilogue, k_rem_segments and k_rem_rows) on the constructed matrices of
tests/tile_cases.py: every case sits on one limit of the tile format -- asserted, on the tiles that are attached, before they are
attached -- in float32, float64 and mixed precision, as K and as K', with every panel-group count of the case.

No tile set that violates the format reaches the library: it does not validate tiles, and a malformed set writes past the LDS
buffer.  ``_engine`` checks the three invariants the kernel trusts (counts <= 15, 64-row totals <= 255, tiles <= cap) on both sides'
tiles in ``before_attach``.

(a) ``test_product``: ``eng.spmv`` against the per-row ``math.fsum`` of the exact float64 products (matrix and vector hold float32
    numbers), within ``(L + 1) u sum_j |K_ij| |v_j|`` plus the smallest normal number, L the row's items (tiles and remainder
    together), u = 2^-24 (float32) or 2^-53 (float64, mixed); rows without items give exactly 0; for cap_and_groups, empties and
    many_groups every group count against the one-launch product within the same bound (the same products in another order);
    detaching gives the CSR kernel's product again, bit for bit.
(b) ``test_epilogue``: an LP around the case matrix (all four bound classes, m_ineq = 2m/5) and the float64 model of the handle
    (tests/handle_model.py) side by side through ``tile_cases.SEQUENCE``, compared after every call at the tolerances of
    tests/test_gpu_sequences.py: A for float64 and mixed, B for float32; after the float32 adaptive step eta within rtol 2e-4 (what
    test_neos3_shaped_instance_matches_oracle holds).  The model decides that step by a margin above 1e-2
    (tests/test_tile_cases_host.py).

The largest error / bound per case, precision and side and the file's wall time are printed at the end (``TILE-EDGE-STATS``) and
written to the file ``PDLP_TILE_EDGE_STATS`` names; profiles/r16_tile_edges/ holds a run."""
import json
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as orc                                   # the checker (tests only)
from tests import tile_cases as tc
from tests.host_lp import DEV
from tests.test_gpu_sequences import A_TOL, B_TOL, Run
from torchpdlp_amd import _native as N

PREC = {"f32": (torch.float32, {}, B_TOL), "f64": (torch.float64, {}, A_TOL),
        "mixed": (torch.float32, dict(vec_dtype=torch.float64, delta=False), A_TOL)}
PARAMS = tc.params()
IDS = [f"{n}-{p}-{s}-g{g}" for n, p, s, g in PARAMS]
STATS = {}                           # "case/precision/side" -> largest error / bound of each check
_REF, _CSR = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _setup():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    orc.set_threads(1)
    N.load()
    t0 = time.time()
    yield
    summary = dict(wall_seconds=round(time.time() - t0, 2), tests=2 * len(PARAMS), worst=STATS)
    print("\nTILE-EDGE-STATS " + json.dumps(summary))
    if os.environ.get("PDLP_TILE_EDGE_STATS"):
        with open(os.environ["PDLP_TILE_EDGE_STATS"], "w") as f:
            json.dump(summary, f, indent=1, sort_keys=True)


def _note(name, prec, side, what, ratio):
    w = STATS.setdefault(f"{name}/{prec}/{side}", {})
    w[what] = max(w.get(what, 0.0), float(ratio))


def _checked(t, lim):
    bad = tc.format_violations(t, lim)
    assert not bad, f"a tile set that violates the format must never be attached: {bad}"
    return t


def _engine(name, prec, side, groups):
    """engine of the LP around the case (side "K": K is the case matrix, "KT": K' is), the case side tiled in ``groups`` panel
    groups with its edge asserted, the other side with the same arguments where it can be tiled"""
    case, lim, lp = tc.get_case(name, prec), tc.LIMITS[prec], tc.get_lp(name, prec, side)
    dtype, kw, _ = PREC[prec]
    edge = 0 if side == "K" else 1
    seen = {}

    def before_attach(tr, t):
        if tr == edge:
            tc.with_groups(t, groups)
        seen[tr] = _checked(t, lim)

    args = [dict(case.args, groups=1), dict(case.args, groups=1)]
    args[edge]["groups"] = groups
    eng = lp.engine(dtype, "tiles", tile_args=tuple(args), before_attach=before_attach, **kw)
    got = eng.tile_limits()
    assert (got["rpt_max"], got["cap"], got["nt"]) == (lim.rpt_max, lim.cap, lim.nt) and got["max_groups"] >= max(case.groups)
    assert edge in seen and seen[edge].groups == groups and eng.tiles[edge] is seen[edge], "the case matrix must be tiled"
    assert ((1 - edge) not in seen) == case.other_side_csr
    for what, holds in case.predicates:
        assert holds(seen[edge]), f"{name} [{prec}] does not hold its edge: {what}"
    assert eng.kernels[edge].startswith("tiled" if groups == 1 else f"tiled/{groups} groups") and ("remainder" in eng.kernels[edge]) == (seen[edge].nrem > 0)
    assert eng.mixed == (prec == "mixed") and not eng.delta
    return eng, lp, case, seen[edge]


def _reference(name, prec):
    """computed once per case matrix, shared, never written to"""
    key = (name, tc.LIMITS[prec])
    if key not in _REF:
        A = tc.get_case(name, prec).A
        v = tc.probe(A.shape[1])
        _REF[key] = (v,) + tc.exact_product(A, v)
    return _REF[key]


def _csr_product(name, prec, side):
    """the CSR kernel's product of the case matrix (an engine that never had tiles)"""
    key = (name, prec, side)
    if key not in _CSR:
        dtype, kw, _ = PREC[prec]
        eng = tc.get_lp(name, prec, side).engine(dtype, "csr", **kw)
        v = _reference(name, prec)[0]
        _CSR[key] = eng.spmv(torch.tensor(v, dtype=eng.dtype, device=DEV), side == "KT").cpu().numpy().astype(np.float64)
    return _CSR[key]


@pytest.mark.parametrize("name,prec,side,groups", PARAMS, ids=IDS)
def test_product(name, prec, side, groups):
    eng, lp, case, t = _engine(name, prec, side, groups)
    v, ref, mag, items = _reference(name, prec)
    assert int(items.sum()) == t.stats["tiled"] + t.nrem
    bound = tc.product_bound(prec, mag, items)
    x = torch.tensor(v, dtype=eng.dtype, device=DEV)
    mul = lambda: eng.spmv(x, side == "KT").cpu().numpy().astype(np.float64)
    got = mul()
    err = np.abs(got - ref)
    worst = int(np.argmax(err / bound))
    print(f"product {name} {prec} {side} g{groups}: largest error / bound {err[worst] / bound[worst]:.3e} (row {worst}, {items[worst]} items)")
    _note(name, prec, side, "product", err[worst] / bound[worst])
    assert np.all(np.isfinite(got)) and np.all(err <= bound), f"row {worst}: |{got[worst]!r} - {ref[worst]!r}| = {err[worst]:.3e} > {bound[worst]:.3e}"
    assert np.all(got[items == 0] == 0), "a row without items"
    assert np.array_equal(mul(), got), "the product is not deterministic"
    edge = 0 if side == "K" else 1
    rp, ci, va = eng.KT if edge else eng.K
    if groups != 1 and name in tc.FUSED_AGAINST_GROUPS:
        lim = eng.tile_limits()
        from torchpdlp_amd.tiled import build_tiles
        fused = build_tiles(rp, ci, va, t.nrows, t.ncols, groups=1, max_groups=lim["max_groups"],
                            kernel_limits=(lim["rpt_max"], lim["cap"], lim["nt"]), **case.args)
        eng.attach_tiles(edge, _checked(fused, tc.LIMITS[prec]))
        assert eng.kernels[edge].startswith("tiled") and "groups" not in eng.kernels[edge]
        one = mul()
        d = np.abs(got - one)
        print(f"  {groups} groups against the one-launch product: {np.max(d / bound):.3e} of the bound")
        _note(name, prec, side, "groups_vs_fused", np.max(d / bound))
        assert np.all(d <= bound) and np.all(np.abs(one - ref) <= bound)
    eng.attach_tiles(edge, None)
    assert eng.kernels[edge] == "csr"
    assert np.array_equal(mul(), _csr_product(name, prec, side)), "detached: not the CSR kernel's product"


class EdgeRun(Run):
    """tests/test_gpu_sequences.py's comparison of an engine with the model, call by call; the ratios go to this file's STATS"""

    def __init__(self, key, prec, *a):
        super().__init__(*a)
        self.key, self.prec, self.adaptive_done = key, prec, False

    def note(self, what, dev, bound):
        assert np.isfinite(dev), self.message(what)
        if bound > 0:
            _note(*self.key, "epilogue", dev / bound)
        assert dev <= bound, self.message(f"{what}: |engine - model| = {dev:.3e} > {bound:.3e}")

    def state(self):
        self.adaptive_done = self.adaptive_done or (self.issued[-1][0] == "iterate" and bool(self.issued[-1][2]))
        x, y = self.eng.get_iterate(N.CUR)
        self.vec("x", x.cpu().numpy(), self.model.x)
        self.vec("y", y.cpu().numpy(), self.model.y)
        got, ref = self.eng.scalars(), self.model.scalars()
        for key in ("eta", "omega", "eta_sum", "w_pending"):
            rel = 2e-4 if (key == "eta" and self.prec == "f32" and self.adaptive_done) else self.tol["iter"]
            self.note(key, abs(got[key] - ref[key]), rel * (abs(ref[key]) if ref[key] else 1.0) if key != "omega" else 1e-7 * ref[key])
        assert got["k"] == ref["k"], self.message(f"k = {got['k']}, model {ref['k']}")


@pytest.mark.parametrize("name,prec,side,groups", PARAMS, ids=IDS)
def test_epilogue(name, prec, side, groups):
    eng, lp, case, t = _engine(name, prec, side, groups)
    cfg = f"{name}-{prec}-{side}-g{groups}"
    run = EdgeRun((name, prec, side), prec, cfg, lp, eng, PREC[prec][2])
    run.run(cfg, tc.SEQUENCE)
    assert run.adaptive_done and eng.scalars()["k"] == 2
