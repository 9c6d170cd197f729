"""The Halpern solve mode on the host: PdhgDriver(halpern=True) over a numpy engine against a straight-line statement of the method,
rules.halpern_weights, and the refusals of the entry functions and of the library (no GPU)."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from torchpdlp_amd import _native as N
from torchpdlp_amd import rules
from torchpdlp_amd.solver import pdlp_algorithm, run_pdlp


class HalpernOracleEngine:
    """what solver.py uses of PdlpEngine in Halpern mode, in numpy: T(z) is the oracle's fixed PDHG step"""

    def __init__(self, o: orc.OracleLP):
        self.o = o
        self.dtype, self.device, self.comm = torch.float32, torch.device("cpu"), None
        self.n, self.m, self.nl, self.ml = o.n, o.m, o.n, o.m
        self.q, self.c = torch.from_numpy(o.q), torch.from_numpy(o.c)
        self.t = np.float32
        self.calls = []

    def set_iterate(self, x, y):
        self.x, self.y = x.numpy().astype(np.float32).copy(), y.numpy().astype(np.float32).copy()
        self.x_last, self.y_last = self.x.copy(), self.y.copy()
        self.xc = self.yc = None
        self.since = 0

    def set_step(self, eta, omega, theta=1.0, iteration=0):
        self.eta, self.omega = self.t(eta), self.t(omega)

    def set_omega(self, omega):
        self.omega = self.t(omega)

    def halpern_iterate(self, iters):
        self.calls.append(int(iters))
        for _ in range(int(iters)):
            a, b = rules.halpern_weights(self.since, self.dtype)
            xc, yc = self.o.step_fixed(self.x, self.y, self.eta, self.omega, 1.0)
            self.x = a * (xc + (xc - self.x)) + b * self.x_last
            self.y = a * (self.t(2) * yc - self.y) + b * self.y_last
            self.xc, self.yc = xc, yc
            self.since += 1

    def iterate(self, iters, adaptive):
        raise AssertionError("the Halpern mode never takes a PDHG iteration")

    flush_average = compute_average = iterate

    def kkt(self, which, omega, unscaled=False):
        x, y = {N.CUR: (self.x, self.y), N.AVG: (self.xc, self.yc)}[which]
        return {k: float(v) for k, v in self.o.kkt(x, y, omega).items()}

    def restart(self, which):
        if which == N.AVG:
            self.x, self.y = self.xc, self.yc
        self.since = 0

    def restart_distance(self):
        return (float(np.sum((self.x_last - self.x).astype(np.float64) ** 2)), float(np.sum((self.y_last - self.y).astype(np.float64) ** 2)))

    def mark_restart_point(self):
        self.x_last, self.y_last = self.x.copy(), self.y.copy()

    def get_iterate(self, which=N.CUR):
        x, y = {N.CUR: (self.x, self.y), N.AVG: (self.xc, self.yc)}[which]
        return torch.from_numpy(x.copy()), torch.from_numpy(y.copy())

    def synchronize(self):
        pass


def halpern_model(o, sigma, tol, primal_update, period=40, max_kkt=100_000):
    """the method, straight down: fixed step, candidate = one PDHG step, reflected Halpern update, the KKT-error restart rules at
    the candidate.  -> (x, k, n, j, restarts, status)"""
    t = np.float32
    q_norm, c_norm = (t(np.sqrt(np.sum(v.astype(np.float64) ** 2))) for v in (o.q, o.c))
    eta, omega = t(0.9) / t(sigma), rules.start_omega(q_norm, c_norm, t)
    x, y = np.zeros(o.n, t), np.zeros(o.m, t)
    k = n = j = 0
    kkt_first, restarts = t(0), []
    while j < max_kkt:
        x0, y0, tt, k_prev = x.copy(), y.copy(), 0, t(np.inf)
        while True:
            a, b = t(np.float64(tt + 1) / np.float64(tt + 2)), t(np.float64(1) / np.float64(tt + 2))
            xc, yc = o.step_fixed(x, y, eta, omega, 1.0)
            x, y = a * (xc + (xc - x)) + b * x0, a * (t(2) * yc - y) + b * y0
            k, tt, j = k + 1, tt + 1, j + 1
            if tt % period:
                continue
            r = {key: float(v) for key, v in o.kkt(xc, yc, omega).items()}
            k_cand, j = t(r["kkt"]), j + 1
            crit = 0 if k_cand <= t(0.2) * kkt_first else 1 if (k_cand <= t(0.8) * kkt_first and k_cand > k_prev) else \
                2 if tt >= 0.36 * k else -1
            k_prev = k_cand
            if crit >= 0:
                restarts.append((crit, tt, 1))
                x, y = xc, yc
                break
        n += 1
        if primal_update:
            omega = rules.primal_weight(float(np.sum((x0 - x).astype(np.float64) ** 2)), float(np.sum((y0 - y).astype(np.float64) ** 2)),
                                        omega, 0.5, t)
        kkt_first = rules.kkt_error(r, omega, t)
        j += 2
        if rules.terminated(r, q_norm, c_norm, tol, t):
            return x, k, n, j, restarts, "Solved"
    return x, k, n, j, restarts, "Unsolved (KKT passes limit exceeded)"


def _lp(g, name):
    a = g.group(name)
    return orc.OracleLP(a["m"], a["n"], a["m_ineq"], a["rowptr"], a["colidx"], a["val"], a["c"], a["q"], a["l"], a["u"])


@pytest.fixture(scope="module", autouse=True)
def _one_thread():
    orc.set_threads(1)


@pytest.mark.parametrize("name", ["mixed_27x32", "mixed_400x300"])
@pytest.mark.parametrize("pw", [False, True], ids=["nopw", "pw"])
def test_driver_runs_the_method_as_stated(golden, name, pw):
    """run_pdlp(halpern=True) over the numpy engine and the straight-line statement take the same path with the same arithmetic:
    every count, the restart list and the final x are equal, exactly.  KKT passes: iterations + one per check + two per restart."""
    g = golden("solve_trace.npz")
    o = _lp(g, name)
    sigma = float(g.group(f"{name}/fixed_nopw")["sigma"])
    eng, trace = HalpernOracleEngine(o), dict(kkt=[], omega=[], restarts=[])
    x, obj, k, n, j, status, _ = run_pdlp(eng, tol=1e-4, verbose=False, primal_update=pw, sigma=sigma, trace=trace, halpern=True)
    xm, km, nm, jm, restarts, sm = halpern_model(o, sigma, 1e-4, pw)
    assert status == "Solved" == sm
    assert (k, n, j) == (km, nm, jm)
    assert trace["restarts"] == restarts
    assert np.array_equal(x.numpy(), xm)
    checks = k // 40
    assert j == k + checks + 2 * n and len(trace["kkt"]) == 3 * checks + n
    assert all(np.isinf(v) for v in trace["kkt"][0::3][:1])               # (kkt_cur of the first check: the three numbers handed over)
    assert sum(eng.calls) == k and max(eng.calls) <= 40
    assert abs(obj - float(g.group(f"{name}/fixed_nopw")["obj"])) <= 2e-3 * (1 + abs(float(g.group(f"{name}/fixed_nopw")["obj"])))
    assert len(trace["omega"]) == (n if pw else 0)


def test_halpern_weights():
    for dt, t in ((np.float32, np.float32), (torch.float32, np.float32), (np.float64, np.float64), (torch.float64, np.float64)):
        a, b = rules.halpern_weights(0, dt)
        assert type(a) is t and type(b) is t and (a, b) == (t(0.5), t(0.5))
        for it in (1, 2, 5, 39, 40, 1000, 123457):
            a, b = rules.halpern_weights(it, dt)
            assert type(a) is t and t(a + b) == t(1)
            # the rounded doubles, each rounded once
            assert a == t(np.float64(it + 1) / np.float64(it + 2)) and b == t(np.float64(1) / np.float64(it + 2))
    a32, _ = rules.halpern_weights(5, np.float32)
    a64, _ = rules.halpern_weights(5, np.float64)
    assert a32 == np.float32(a64) and float(a32) != float(a64)


REFUSED = [dict(adaptive=True), dict(adaptive=True, adaptive_retry=True), dict(infeasibility_detect=True), dict(precision="mixed"),
           dict(comm=True)]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: "+".join(kw))
def test_refused_combinations_raise_before_any_device_work(kw):
    """adaptive, adaptive_retry, infeasibility_detect, mixed precision and a communicator have no Halpern form: ValueError from
    pdlp_algorithm and from solve_lp, on a machine without a device (nothing is put anywhere before the check)"""
    import torchpdlp_amd as tp
    K = torch.eye(3)
    v = torch.zeros(3)
    with pytest.raises(ValueError, match="halpern"):
        pdlp_algorithm(K, 1, v, v, v, v + 1, "cpu", verbose=False, halpern=True, **kw)
    names = dict(adaptive="adaptive_stepsize")
    with pytest.raises(ValueError, match="halpern"):
        tp.solve_lp((v, K, v, 1, v, v + 1), device="cpu", halpern=True, **{names.get(k, k): val for k, val in kw.items()})


def test_driver_refuses_too():
    """run_pdlp / PdhgDriver over an existing engine: the same refusal, before the engine is touched"""
    class Untouchable:
        comm, mixed = None, False

        def __getattr__(self, name):
            raise AssertionError(f"engine.{name} was used")
    with pytest.raises(ValueError, match="halpern"):
        run_pdlp(Untouchable(), verbose=False, halpern=True, adaptive=True, sigma=1.0)
    with pytest.raises(ValueError, match="halpern"):
        run_pdlp(Untouchable(), verbose=False, halpern=True, infeasibility_detect=True, sigma=1.0)


def test_library_entry_point():
    lib = N.load()
    assert "pdlp_halpern_iterate" in N.SIGNATURES and N.ABI_VERSION == 18
    assert lib.pdlp_halpern_iterate(None, 1) == -1
    assert lib.pdlp_abi_version() == 18


def test_cli_has_the_flag():
    from torchpdlp_amd.__main__ import COLUMNS, parse_args
    assert parse_args(["--halpern"]).halpern is True and parse_args([]).halpern is False
    assert len(COLUMNS) == 7
