"""Call sequences against the float64 model of the handle (tests/handle_model.py): a PdlpEngine is driven through the 40 seeded random
sequences of the documented call grammar and through the directed list (one hand-written sequence per transition of the flags that
say whether a carried product still belongs to its vector), and after EVERY call what the engine returns -- or, for a call that
returns nothing, its current iterate and scalar block -- is compared with the model, which carries nothing and multiplies every
product out in float64.  A forgotten invalidation shows as a product that is one iterate stale: at least 1e-4 away
(tests/test_sequences_host.py), 10^4 tolerances or more in float64.

Tolerances (|engine - model| <= tol * scale; scale = 1 + max|model vector|, or 1 + |p| + |d_adj| for the numbers of a KKT pass):
  A  float64: iterates and scalars 1e-10, KKT / report / product numbers 1e-9.  The suite holds 1e-11 / 1e-10 for 20 float64
     iterations against this oracle (test_mixed_precision_matches_the_float64_oracle); sequences here are up to three times as long,
     use sum-formed products, and the adaptive rule grows last-bit differences about 10^5-fold over 40 steps (measured there:
     0.7 % in float32), about 2e-11 in float64.
  B  float32 (fixed-step and Halpern periods): 5e-5, what test_restart_check_from_running_products holds for fixed steps.
  C  delta mode: the bounds of test_delta_mode_rounding_scales_with_the_step at scale 1, each measured as that test measures it.
     Iterates (CUR after every call that returns nothing; the evaluated iterate at every KKT pass and report) against the MODEL's
     within 3e-6 * max(1, step), step = the largest move of an entry since the last set_iterate.  pr, dr, p, d_adj of a KKT pass or
     a report against the float64 evaluation of the ENGINE's own iterate -- as that test does with o.kkt(px, py) of the engine's
     buffers -- within rtol 1e-6 + 1e-6: the bound is about the pass (products from the anchors and float32 differences), a stale
     or wrong anchor is 1e-4 or more away from it, and the iterate's own deviation, which K carries into these numbers and which
     grows with the step, has its bound above.  A report multiplies out (float64 sums over the float32 matrix): its vectors against
     the same evaluation within 1e-9 like the float64 products.  Derived from the iterate bound d (not set by the issue): squared
     restart distances within 2 |dist| |e| + |e|^2 with |e| = 2 d sqrt(length), the step size within 2e-5 (a ratio of sums of
     squared step entries, each relative 3e-6 or worse: four such factors), the infeasibility detector's status only.
"""
import json
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as orc                                   # the checker (tests only)
from tests import handle_model as hm
from tests.host_lp import DEV, get_lp
from torchpdlp_amd import _native as N

WHICH = {hm.CUR: N.CUR, hm.AVG: N.AVG, hm.PREV: N.PREV}
A_TOL, B_TOL = dict(iter=1e-10, kkt=1e-9), dict(iter=5e-5, kkt=5e-5)
NO_RETRY_HALPERN = dict(retry=False, halpern=False, graph_toggle=False)
# id -> (LP, engine dtype, product form, engine keywords, environment, grammar, tolerance)
CONFIGS = {
    "f64-csr": ("seq", torch.float64, "csr", {}, {}, {}, A_TOL),
    "f64-tiles_groups": ("mid_scaled", torch.float64, "tiles_groups", {}, {}, {}, A_TOL),
    "f64-csr-norunning": ("seq", torch.float64, "csr", {}, {"PDLP_RUNNING_KKT": "0", "PDLP_NO_KTY_REUSE": "1"}, {}, A_TOL),
    "f64-csr-graph": ("seq", torch.float64, "csr", {}, {"PDLP_GRAPH": "1"}, NO_RETRY_HALPERN, A_TOL),
    "f32-csr": ("seq", torch.float32, "csr", {}, {}, dict(adaptive=False, retry=False), B_TOL),
    "mixed-delta": ("seq", torch.float32, "csr", dict(vec_dtype=torch.float64, delta=True), {}, dict(NO_RETRY_HALPERN, delta=True), "C"),
}
STATS = {}                           # configuration -> largest deviation / tolerance seen, and where; wall time


@pytest.fixture(scope="module", autouse=True)
def _setup():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    orc.set_threads(1)
    N.load()
    t0 = time.time()
    yield
    summary = dict(wall_seconds=round(time.time() - t0, 2), worst=STATS)
    print("\nSEQUENCE-STATS " + json.dumps(summary))
    if os.environ.get("PDLP_SEQUENCE_STATS"):
        with open(os.environ["PDLP_SEQUENCE_STATS"], "w") as f:
            json.dump(summary, f, indent=1)


def _fits_delta(calls):
    """at most 12 iterations after a set_iterate (the premise of tolerance C; refresh_products makes the anchors exact again, not
    the iterate, so it does not start the count again: stricter than one count per refresh)"""
    n = 0
    for c in calls:
        n = 0 if c[0] == "set_iterate" else n + (c[1] if c[0] == "iterate" else 0)
        if n > 12:
            return False
    return True


def sequence_names(cfg):
    feats = CONFIGS[cfg][5]
    names = [f"seed{s}" for s in hm.SEEDS]
    return names + [k for k, calls in hm.DIRECTED.items() if hm.restricted(calls, feats) and (not feats.get("delta") or _fits_delta(calls))]


class Run:
    """one engine and one model side by side"""

    def __init__(self, cfg, lp, eng, tol):
        self.cfg, self.lp, self.eng, self.tol = cfg, lp, eng, tol
        self.model = hm.HandleModel(lp)
        self.t = lambda v: torch.tensor(np.asarray(v), dtype=eng.dtype, device=DEV)
        self.issued = []
        self.start = (self.model.x, self.model.y)
        self.delta = dict(delta=True, anchors_valid=False, dy_folded=False) if tol == "C" else None
        self.cand_avg = False        # delta mode: a KKT pass at the average has left its products (the anchors a restart adopts)

    # ---- the engine's side of a call --------------------------------------------------------------
    def engine_call(self, call):
        e, name, a = self.eng, call[0], call[1:]
        host = lambda v: v.detach().cpu().numpy().astype(np.float64)
        if name == "set_iterate":
            x, y = hm.start_point(self.lp, a[0])
            return e.set_iterate(self.t(x), self.t(y))
        if name == "set_step":
            return e.set_step(a[0] * self.model.eta0, a[1], 1.0, a[2])
        if name == "kkt":
            return e.kkt(WHICH[a[0]], a[1], a[2])
        if name == "report":
            r = e.report(WHICH[a[0]], a[1], a[2])
            return {k: (host(v) if isinstance(v, torch.Tensor) else v) for k, v in r.items()}
        if name == "restart":
            return e.restart(WHICH[a[0]])
        if name == "get_iterate":
            return tuple(host(v) for v in e.get_iterate(WHICH[a[0]]))
        if name == "detect_infeasibility":
            status, diag = e.detect_infeasibility(a[0], diagnostics=True)
            return status, np.array(diag)
        if name == "spmv":
            return host(e.spmv(self.t(hm.probe_vector(self.lp, a[0], a[1])), a[1]))
        if name == "power_iteration":
            return e.power_iteration(self.t(hm.probe_vector(self.lp, a[0], False)), a[1])
        if name == "set_option":
            if self.cfg != "f64-csr-norunning":      # (that configuration keeps both switches off)
                e.set_option(getattr(N, "OPT_" + a[0]), a[1])
            return None
        if name == "refused":
            with pytest.raises(N.PdlpError, match="call sequence"):
                getattr(e, a[0])(*a[1:]) if a[0] != "flush_average" else e.flush_average(False)
            return None
        return getattr(e, name)(*a)

    # ---- comparisons ------------------------------------------------------------------------------
    def note(self, what, dev, bound):
        assert np.isfinite(dev), self.message(what)
        w = STATS.setdefault(self.cfg, dict(ratio=0.0))
        if bound > 0 and dev / bound > w["ratio"]:
            w.update(ratio=float(dev / bound), deviation=float(dev), bound=float(bound), what=what, sequence=self.name, call=len(self.issued))
        assert dev <= bound, self.message(f"{what}: |engine - model| = {dev:.3e} > {bound:.3e}")

    def message(self, text):
        return f"{self.cfg} {self.name} after {len(self.issued)} calls: {text}\ncalls = {self.issued!r}"

    def iterate_bound(self):
        """delta mode: 3e-6 * max(1, step)"""
        step = max(np.abs(self.model.x - self.start[0]).max(), np.abs(self.model.y - self.start[1]).max())
        return 3e-6 * max(1.0, step)

    def vec(self, what, got, ref, kind="iter", bound=None):
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        assert got.shape == ref.shape, self.message(what)
        if bound is None:
            bound = self.iterate_bound() if self.tol == "C" else self.tol[kind] * (1.0 + (np.abs(ref).max() if ref.size else 0.0))
        self.note(what, float(np.abs(got - ref).max()) if ref.size else 0.0, bound)

    def kkt_numbers(self, what, got, ref):
        if self.tol == "C":
            for key in ("pr", "dr", "p", "d_adj"):
                self.note(f"{what}:{key}", abs(got[key] - ref[key]), 1e-6 + 1e-6 * abs(ref[key]))
            return
        scale = 1.0 + abs(ref["p"]) + abs(ref["d_adj"])
        for key in ("pr", "dr", "gap", "p", "d_adj", "kkt"):
            self.note(f"{what}:{key}", abs(got[key] - ref[key]), self.tol["kkt"] * scale)

    def compare(self, call, got, ref):
        name = call[0]
        if name == "kkt":
            self.kkt_numbers(f"kkt({call[1]})", got, ref)
        elif name == "report":
            self.kkt_numbers(f"report({call[1]})", got, ref)
            exact = self.tol == "C"      # (ref is then the evaluation of the engine's own iterate: run())
            self.vec("report y", got["y"], ref["y"], "iter", 1e-12 * (1 + np.abs(ref["y"]).max()) if exact else None)
            for key in ("reduced_costs", "row_activity"):
                self.vec(f"report {key}", got[key], ref[key], "kkt", 1e-9 * (1 + np.abs(ref[key]).max()) if exact else None)
        elif name == "get_iterate":
            self.vec(f"x of {call[1]}", got[0], ref[0])
            self.vec(f"y of {call[1]}", got[1], ref[1])
        elif name == "restart_distance":
            for what, g, r, ln in (("dx2", got[0], ref[0], self.lp.n), ("dy2", got[1], ref[1], self.lp.m)):
                if self.tol == "C":
                    e = 2 * self.iterate_bound() * np.sqrt(ln)
                    self.note(what, abs(g - r), 2 * np.sqrt(r) * e + e * e)
                else:
                    self.note(what, abs(g - r), self.tol["kkt"] * (1.0 + abs(r)))
        elif name == "spmv":
            self.vec("spmv", got, ref, "kkt", 1e-9 * (1 + np.abs(ref).max()) if self.tol == "C" else None)
        elif name == "power_iteration":
            self.note("power_iteration", abs(got - ref), (1e-9 if self.tol == "C" else self.tol["kkt"]) * (1.0 + abs(ref)))
        elif name == "detect_infeasibility":
            (st, diag), (so, dgo), tol = got, ref, call[1]
            margins = [abs(dgo[0] - tol), abs(dgo[2] - tol), abs(dgo[4] - tol), abs(dgo[6] - dgo[7] + tol)]
            if min(margins) > 1e-4 * max(1.0, tol):           # (no threshold within rounding of the tested quantity)
                assert st == so, self.message(f"infeasibility status {st} != {so}")
            if self.tol is A_TOL:
                self.vec("infeasibility sums", diag, dgo, "kkt")
            elif self.tol is B_TOL:                           # (the three counts may flip on an entry next to its threshold)
                self.vec("infeasibility sums", diag[[0, 2, 4, 6, 7]], dgo[[0, 2, 4, 6, 7]], "kkt", 5e-5 * (1 + np.abs(dgo).max()))

    def state(self):
        """what a caller can see of the handle after a call that returns nothing"""
        x, y = self.eng.get_iterate(N.CUR)
        self.vec("x", x.cpu().numpy(), self.model.x)
        self.vec("y", y.cpu().numpy(), self.model.y)
        got, ref = self.eng.scalars(), self.model.scalars()
        rel = 2e-5 if self.tol == "C" else self.tol["iter"]
        for key in ("eta", "omega", "eta_sum", "w_pending"):
            self.note(key, abs(got[key] - ref[key]), rel * (abs(ref[key]) if ref[key] else 1.0) if key != "omega" else 1e-7 * ref[key])
        assert got["k"] == ref["k"], self.message(f"k = {got['k']}, model {ref['k']}")

    def expect_delta(self, call):
        d, name = self.delta, call[0]
        if name == "set_iterate":
            d.update(anchors_valid=False, dy_folded=False)
            self.cand_avg = False
        elif name in ("refresh_products", "kkt"):
            d.update(anchors_valid=True, dy_folded=True)
            self.cand_avg = self.cand_avg or (name == "kkt" and call[1] == hm.AVG)
        elif name == "iterate":
            d.update(anchors_valid=True, dy_folded=False)
            self.cand_avg = False
        elif name == "restart":
            if call[1] == hm.AVG:
                d.update(dy_folded=True) if self.cand_avg else d.update(anchors_valid=False)
            self.cand_avg = False
        assert self.eng.delta_state() == d, self.message(f"delta_state {self.eng.delta_state()} != {d}")

    # ---- a sequence -------------------------------------------------------------------------------
    def run(self, name, calls):
        self.name = name
        self.eng.infeas_reset()
        for call in calls:
            self.issued.append(call)
            ref = self.model.apply(call)
            got = self.engine_call(call)
            if call[0] == "set_iterate":
                self.start = (self.model.x, self.model.y)
            if self.tol == "C" and call[0] in ("kkt", "report"):
                # tolerance C: the evaluated iterate against the model's, the numbers against the evaluation of that very iterate
                x, y = (v.cpu().numpy() for v in self.eng.get_iterate(WHICH[call[1]]))
                mx, my = self.model.get_iterate(call[1])
                self.vec(f"x of {call[1]}", x, mx)
                self.vec(f"y of {call[1]}", y, my)
                ref = self.model.kkt_at(x, y, call[2], call[3]) if call[0] == "kkt" else self.model.report_at(x, y, call[2], call[3])
            if ref is None:
                self.state()
            else:
                self.compare(call, got, ref)
            if call[0] == "iterate" and call[2] and call[1] == 1 and self.tol != "C":
                acc = self.eng.scalars()["accepted"]
                assert bool(acc) == self.model.accepted, self.message(f"accepted = {acc}, model {self.model.accepted}")
            if self.delta is not None:
                self.expect_delta(call)
            if self.cfg == "f64-csr-graph" and call[0] in ("iterate", "restart"):
                # graph replay: no retry and no Halpern iteration -- refused, and nothing changes
                for refused in (self.eng.adaptive_retry, lambda: self.eng.halpern_iterate(1)):
                    with pytest.raises(N.PdlpError, match="call sequence"):
                        refused()
                self.state()


def _sequence(cfg, name, lp):
    if name.startswith("seed"):
        return hm.generate(lp, int(name[4:]), CONFIGS[cfg][5])
    return hm.DIRECTED[name]


def pytest_generate_tests(metafunc):
    if "cfg" in metafunc.fixturenames:
        metafunc.parametrize("cfg,name", [(c, n) for c in CONFIGS for n in sequence_names(c)], ids=lambda v: v)


def test_sequence(cfg, name, monkeypatch):
    lp_name, dtype, form, kw, env, _, tol = CONFIGS[cfg]
    for k in ("PDLP_RUNNING_KKT", "PDLP_NO_KTY_REUSE", "PDLP_GRAPH", "PDLP_DELTA", "PDLP_TILED", "PDLP_SORTED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lp = get_lp(lp_name)
    eng = lp.engine(dtype, form, **kw)
    if cfg == "mixed-delta":
        assert eng.mixed and eng.delta
    Run(cfg, lp, eng, tol).run(name, _sequence(cfg, name, lp))
