"""A float64 model of a single-LP handle (include/pdlp_hip.h) and call sequences to run against it -- no GPU.

``HandleModel`` holds what the header says a handle holds -- the current, previous and averaged (or Halpern candidate) iterates, the
eta-weighted sums with ``eta_sum`` and the weight still pending, the restart point, eta / omega / theta / k, the Halpern count t and
the infeasibility detector's ``lam_prev`` -- and NOTHING carried: every product is multiplied out in float64 from the vectors it
belongs to at the moment it is needed.  The engine saves those products by carrying them along; which of them still belongs to its
vector is the state of one struct (``Carried`` in pdlp_handle.inc, whose comment holds the rules and whose member functions are the
only writers); whatever order the calls come in, inside the documented contract, its numbers must stay the model's.
The steps are the float64 oracle's (``step_fixed`` / ``step_adaptive`` / ``kkt`` / ``detect_infeasibility``), the Halpern step is the
formula of ``pdlp_halpern_iterate``'s comment, the averaging is pdhg.py:107-119 as ``oracle.pdlp_algorithm`` restates it (adaptive:
an iterate's weight is known one step later, so it is PENDING until the next iteration or ``flush_average(True)`` adds its term; the
scalar ``eta_sum`` has it at once -- both are what ``pdlp_get_scalars`` shows).

A call is a tuple ``(name, *arguments)`` of plain numbers and strings, so a failing sequence printed by a test can be pasted into
``DIRECTED``: vectors are named by the seed they are drawn from, eta by its factor on 0.9 / ||K||_2.  ``HandleModel.apply`` runs
one; tests/test_gpu_sequences.py has the same for a PdlpEngine.

The grammar (``generate``): every sequence starts ``set_iterate; set_step``.  A period -- from a ``set_iterate`` or ``restart`` to the
next -- has ONE mode, fixed-step, adaptive or Halpern; ``flush_average``'s flag is the period's mode; ``compute_average`` needs
``eta_sum > 0``; AVG is evaluated or adopted only after a ``compute_average`` or a Halpern iteration of this period; PREV (and the
infeasibility detector, which reads it) only after a PDHG iteration since the last ``set_iterate`` / ``restart`` / ``adaptive_retry``;
after Halpern iterations the two averaging calls are REFUSED until ``set_iterate`` (issued as ``("refused", name)``: the engine must
raise, the model does nothing); iteration counts are 1, 2, 3, 5, 8; ``set_omega`` and the option switches come anywhere; a changed
eta comes at period starts (mid-period only in ``DIRECTED``: that one used to break the running K'y sum).

``adaptive_retry``: the header allows it "after an adaptive iteration whose trial was REJECTED" and nowhere else, so the grammar
draws it only straight after a single adaptive iteration that the model reports as rejected.  (pdlp_adaptive_retry itself does not
look at the flag and would undo an accepted step the same way; that is not promised, so it is not tested.)

Two things the model does that the header does not spell out, each used by one directed sequence only: after ``restart(AVG)`` the
AVG slot holds the iterate that was current (the buffers swap), and ``set_iterate`` keeps eta, omega and k.
"""
from collections import Counter

import numpy as np

CUR, AVG, PREV = "CUR", "AVG", "PREV"
ITERS = (1, 2, 3, 5, 8)
# the 18 calls of the grammar (scalars() is how a test looks at the handle after a call that returns nothing)
CALLS = ("set_iterate", "set_step", "set_omega", "iterate", "halpern_iterate", "adaptive_retry", "flush_average", "compute_average",
         "kkt", "report", "restart", "restart_distance", "mark_restart_point", "infeas_reset", "detect_infeasibility", "spmv",
         "power_iteration", "get_iterate")
FULL = dict(adaptive=True, retry=True, halpern=True, delta=False, graph_toggle=True)    # what a configuration's grammar may use


def project_lambda_box(g, l, u):
    """helpers.py:3-39"""
    lo, hi = np.isneginf(l), np.isposinf(u)
    out = g.copy()
    out[lo & hi] = 0.0
    out[lo & ~hi] = np.minimum(g[lo & ~hi], 0.0)
    out[hi & ~lo] = np.maximum(g[hi & ~lo], 0.0)
    return out


def start_point(lp, seed):
    """away from the optimum: random normal, clipped to the bounds (y >= 0 on the inequality rows)"""
    rng = np.random.default_rng(1000 + int(seed))
    x = np.clip(rng.standard_normal(lp.n), lp.l, lp.u)
    y = rng.standard_normal(lp.m)
    y[:lp.m_ineq] = np.abs(y[:lp.m_ineq])
    return x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)


def probe_vector(lp, seed, transpose):
    v = np.random.default_rng(2000 + int(seed)).standard_normal(lp.m if transpose else lp.n)
    return v.astype(np.float32).astype(np.float64)


class HandleModel:
    def __init__(self, lp):
        self.lp = lp
        self.o = lp.oracle(np.float64)
        self.eta0 = 0.9 / lp.norm2()
        z = np.zeros
        self.x, self.y = z(lp.n), z(lp.m)
        self.xp = self.yp = self.xa = self.ya = None
        self.x_sum, self.y_sum, self.eta_sum, self.eta_sum_before, self.w_pending = z(lp.n), z(lp.m), 0.0, 0.0, 0.0
        self.x_last, self.y_last = z(lp.n), z(lp.m)
        self.eta, self.omega, self.theta, self.k, self.t = 0.0, 1.0, 1.0, 0, 0
        self.lam_prev = z(lp.n)
        self.accepted = True
        self.margins = []            # (what, relative distance): see test_sequences_host.py, the discrimination condition

    # ---- state ------------------------------------------------------------------------------------
    def _zero_sums(self):
        self.x_sum, self.y_sum = np.zeros(self.lp.n), np.zeros(self.lp.m)
        self.eta_sum = self.w_pending = 0.0
        self.t = 0

    def set_iterate(self, x, y):
        self.x, self.y = np.array(x, np.float64), np.array(y, np.float64)
        self.x_last, self.y_last = self.x.copy(), self.y.copy()
        self.xp = self.yp = self.xa = self.ya = None
        self._zero_sums()

    def set_step(self, eta, omega, theta=1.0, iteration=0):
        self.eta, self.omega, self.theta, self.k = float(eta), float(omega), float(theta), int(iteration)

    def set_omega(self, omega):
        self.omega = float(omega)

    def scalars(self):
        return dict(eta=self.eta, omega=self.omega, eta_sum=self.eta_sum, w_pending=self.w_pending, k=float(self.k))

    def get_iterate(self, which=CUR):
        x, y = {CUR: (self.x, self.y), AVG: (self.xa, self.ya), PREV: (self.xp, self.yp)}[which]
        assert x is not None, f"{which} is not defined here: the sequence leaves the contract"
        return x, y

    # ---- iterations -------------------------------------------------------------------------------
    def _margin(self, what, a, b):
        self.margins.append((what, float(np.max(np.abs(a - b)) / (1.0 + np.max(np.abs(a))))))

    def _moved(self, xn, yn):
        A = self.lp.A
        self._margin("kty", A.T @ yn, A.T @ self.y)
        self._margin("kx", A @ xn, A @ self.x)

    def iterate(self, n, adaptive):
        for _ in range(int(n)):
            if adaptive:
                xn, yn, w, eta_hat, info = self.o.step_adaptive(self.x, self.y, self.eta, self.omega, self.theta, self.k + 1)
                self.x_sum = self.x_sum + self.w_pending * self.x          # the weight of the PREVIOUS iterate, known only now
                self.y_sum = self.y_sum + self.w_pending * self.y
                self.w_pending, self.eta, self.accepted = float(w), float(eta_hat), bool(info["accepted"])
            else:
                xn, yn = self.o.step_fixed(self.x, self.y, self.eta, self.omega, self.theta)
                self.x_sum = self.x_sum + self.eta * xn
                self.y_sum = self.y_sum + self.eta * yn
                w = self.eta
            self._moved(xn, yn)
            self.eta_sum_before, self.eta_sum = self.eta_sum, self.eta_sum + float(w)
            self.xp, self.yp, self.x, self.y = self.x, self.y, xn, yn
            self.k += 1
            self.t += 1

    def adaptive_retry(self):
        """the trial is discarded: the old (x, y) is current again, its weight (which the trial's half-steps folded into the sums)
        stays, the trial's leaves eta_sum, k goes back, eta keeps the rule's eta'"""
        self.x, self.y, self.xp, self.yp = self.xp, self.yp, None, None
        self.eta_sum, self.w_pending = self.eta_sum_before, 0.0
        self.k -= 1
        self.t = max(self.t - 1, 0)

    def halpern_iterate(self, n):
        for _ in range(int(n)):
            a, b = (self.t + 1) / (self.t + 2), 1 / (self.t + 2)
            xc, yc = self.o.step_fixed(self.x, self.y, self.eta, self.omega, 1.0)
            xn, yn = a * (xc + (xc - self.x)) + b * self.x_last, a * (2 * yc - self.y) + b * self.y_last
            self._moved(xn, yn)
            if self.t >= 1:          # (at t = 0 from the anchor itself, z+ = (2z' - z + z) / 2 IS the candidate)
                self._margin("kty_avg", self.lp.A.T @ yc, self.lp.A.T @ yn)
                self._margin("kx_avg", self.lp.A @ xc, self.lp.A @ xn)
            self.x, self.y, self.xa, self.ya, self.xp, self.yp = xn, yn, xc, yc, None, None
            self.t += 1

    # ---- restart machinery ------------------------------------------------------------------------
    def flush_average(self, adaptive):
        if adaptive:
            self.x_sum = self.x_sum + self.w_pending * self.x
            self.y_sum = self.y_sum + self.w_pending * self.y
            self.w_pending = 0.0

    def compute_average(self):
        self.xa, self.ya = self.x_sum / self.eta_sum, self.y_sum / self.eta_sum
        if self.t >= 2:              # (after ONE iteration the average IS the current iterate)
            self._margin("kty_avg", self.lp.A.T @ self.ya, self.lp.A.T @ self.y)
            self._margin("kx_avg", self.lp.A @ self.xa, self.lp.A @ self.x)

    def kkt_at(self, x, y, omega, unscaled=False):
        """compute_residuals_and_duality_gap + KKT_error of any point (of the un-preconditioned LP at (D_col x, D_row y))"""
        o = self.lp.unscaled_oracle() if unscaled else self.o
        x, y = (self.lp.d_col * x, self.lp.d_row * y) if unscaled else (x, y)
        return {k: float(v) for k, v in o.kkt(x, y, omega).items()}

    def report_at(self, x, y, unscaled=False, omega=1.0):
        o = self.lp.unscaled_oracle() if unscaled else self.o
        xs, ys = (self.lp.d_col * x, self.lp.d_row * y) if unscaled else (x, y)
        A = o.scipy()
        return dict(y=ys, reduced_costs=project_lambda_box(o.c - A.T @ ys, o.l, o.u), row_activity=A @ xs, **self.kkt_at(x, y, omega, unscaled))

    def kkt(self, which, omega, unscaled=False):
        return self.kkt_at(*self.get_iterate(which), omega, unscaled)

    def report(self, which=CUR, unscaled=False, omega=1.0):
        return self.report_at(*self.get_iterate(which), unscaled, omega)

    def restart(self, which):
        if which == AVG:
            self.x, self.y, self.xa, self.ya = self.xa, self.ya, self.x, self.y
        self._zero_sums()

    def restart_distance(self):
        return float(np.sum((self.x - self.x_last) ** 2)), float(np.sum((self.y - self.y_last) ** 2))

    def mark_restart_point(self):
        self.x_last, self.y_last = self.x.copy(), self.y.copy()

    def infeas_reset(self):
        self.lam_prev = np.zeros(self.lp.n)

    def detect_infeasibility(self, tol):
        xp, yp = self.get_iterate(PREV)
        status, lam, diag = self.o.detect_infeasibility(self.x, self.y, xp, yp, self.lam_prev, tol)
        self.lam_prev = lam
        return status, np.array(diag, np.float64)

    def spmv(self, v, transpose=False):
        return (self.lp.A.T if transpose else self.lp.A) @ np.asarray(v, np.float64)

    def power_iteration(self, b0, iters):
        return float(self.o.power_iter(b0, iters))

    # ---- one call of a sequence -------------------------------------------------------------------
    def apply(self, call):
        name, args = call[0], call[1:]
        if name == "set_iterate":
            return self.set_iterate(*start_point(self.lp, args[0]))
        if name == "set_step":
            return self.set_step(args[0] * self.eta0, args[1], 1.0, args[2])
        if name == "spmv":
            return self.spmv(probe_vector(self.lp, args[0], args[1]), args[1])
        if name == "power_iteration":
            return self.power_iteration(probe_vector(self.lp, args[0], False), args[1])
        if name in ("set_option", "refused", "refresh_products"):
            return None              # (nothing the header lets a caller see changes)
        return getattr(self, name)(*args)


# ---------------------------------------------------------------------------------------------------------------------
# what the handle may be asked next: the contract of the module docstring, followed over a list of calls
# ---------------------------------------------------------------------------------------------------------------------
class Contract:
    """the few facts the grammar needs, from the calls alone (plus, for adaptive_retry, whether the model rejected the step)"""

    def __init__(self):
        self.mode = None             # of this period: "fixed" | "adaptive" | "halpern"; None until its first iteration
        self.its = 0                 # iterations of this period
        self.avg = self.prev = False
        self.halpern_since_set = False
        self.retry_ok = False
        self.weight = False          # eta_sum > 0
        self.since_exact = 0         # delta mode: iterations since engine and model last held the same iterate (set_iterate)
        self.since_refresh = 0       # ... and since the anchors were last recomputed

    def after(self, call, rejected=False):
        name = call[0]
        self.retry_ok = False
        if name == "set_iterate":
            self.__init__()
        elif name == "restart":
            self.mode, self.its, self.avg, self.prev, self.weight = None, 0, False, False, False
        elif name == "iterate":
            self.mode = "adaptive" if call[2] else "fixed"
            self.its += call[1]
            self.since_exact += call[1]
            self.since_refresh += call[1]
            self.prev = self.weight = True
            self.retry_ok = bool(call[2]) and call[1] == 1 and rejected
        elif name == "halpern_iterate":
            self.mode, self.avg, self.prev, self.halpern_since_set = "halpern", True, False, True
            self.its += call[1]
        elif name == "adaptive_retry":
            self.its -= 1
            self.prev = False
            self.weight = self.its > 0
        elif name == "compute_average":
            self.avg = True
        elif name == "refresh_products":
            self.since_refresh = 0

    def defined(self, which):
        return which == CUR or (which == AVG and self.avg) or (which == PREV and self.prev)


def generate(lp, seed, features=FULL, model=None):
    """one random sequence of 22 to 30 grammar calls (the ("refused", ...) and ("set_option", ...) entries come on top).
    Grammars with adaptive_retry take long steps late in a solve to meet rejected trials; the live rule keeps a rejected step, so
    about half of those sequences leave the region where the iteration converges and their iterates grow (1e3 to 1e18).  Every
    bound the tests hold is relative to the size of what it bounds, and so is the distance of a stale product."""
    rng = np.random.default_rng(seed)
    f = dict(FULL, **features)
    model = model or HandleModel(lp)
    ct, calls = Contract(), []
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    omega = lambda: float(np.float32(rng.uniform(0.5, 2.0)))

    def emit(call):
        calls.append(call)
        model.apply(call)
        ct.after(call, rejected=call[0] == "iterate" and bool(call[2]) and not model.accepted)

    emit(("set_iterate", int(rng.integers(100))))
    late_step = lambda: ("set_step", 8.0, omega(), int(pick((1000, 100000))))
    emit(late_step() if (f["retry"] and rng.random() < 0.7) else ("set_step", 1.0, omega(), 0))
    length, count = int(rng.integers(22, 31)), 2
    while count < length:
        modes = [m for m in ("fixed", "adaptive", "halpern") if f.get(m, True)]
        if ct.mode is not None:
            modes = [ct.mode]
        which = [w for w in (CUR, AVG, PREV) if ct.defined(w)]
        ops = {"iterate": 9.0, "kkt": 4.5, "set_omega": 1.8, "report": 2.0, "spmv": 1.4, "power_iteration": 2.0, "get_iterate": 2.0,
               "infeas_reset": 2.4, "restart": 2.2, "restart_distance": 2.4, "mark_restart_point": 1.8, "set_iterate": 0.5,
               "set_option": 0.5}
        if ct.its == 0 and ct.mode is None:
            ops["set_step"] = 2.0
        if ct.mode in ("fixed", "adaptive") and ct.its > 0 and not ct.halpern_since_set:
            ops["flush_average"] = 3.0
        if ct.mode != "halpern" and not ct.halpern_since_set and ct.weight:
            ops["compute_average"] = 3.0
        if ct.prev:
            ops["detect_infeasibility"] = 5.5
        if ct.halpern_since_set:
            ops["refused"] = 0.8
        if f["delta"] and ct.its == 0 and ct.since_refresh > 0:
            ops["refresh_products"] = 4.0
        if ct.retry_ok and f["retry"]:
            ops = {"adaptive_retry": 8.0, "kkt": 1.0}
        names = sorted(ops)
        p = np.array([ops[n] for n in names])
        name = names[int(rng.choice(len(names), p=p / p.sum()))]
        if name == "iterate":
            long_step = model.eta > 1.01 * model.eta0        # (only the adaptive rule may run with it: it shrinks it)
            mode = "adaptive" if ("adaptive" in modes and long_step and rng.random() < 0.8) else pick(modes)
            if mode != "adaptive" and long_step:
                assert ct.mode is None and ct.its == 0       # a period starts: a step inside the convergent range first
                emit(("set_step", float(pick((1.0, 0.5))), omega(), int(model.k)))
                count += 1
                continue
            n = 1 if (mode == "adaptive" and f["retry"] and rng.random() < (0.9 if model.k >= 1000 else 0.4)) else int(pick(ITERS))
            if f["delta"] and ct.since_exact + n > 12:
                if ct.since_exact < 12:
                    n = max(i for i in ITERS if ct.since_exact + i <= 12)
                else:
                    emit(("set_iterate", int(rng.integers(100))))
                    count += 1
                    continue
            call = ("halpern_iterate", n) if mode == "halpern" else ("iterate", n, mode == "adaptive")
        elif name == "kkt":
            w = pick(which)
            call = ("kkt", w, omega(), bool(rng.random() < 0.3) and not (f["delta"] and w != CUR))
        elif name == "report":
            call = ("report", pick(which), bool(rng.random() < 0.3), omega())
        elif name == "get_iterate":
            call = ("get_iterate", pick(which))
        elif name == "restart":
            call = ("restart", AVG if (ct.avg and rng.random() < 0.7) else CUR)
        elif name == "set_step":
            # (an adaptive period that starts with a long step late in a solve meets rejected trials: the rule then keeps eta
            # within (k + 1)^-0.3 of eta_bar, which moves more than that from one step to the next)
            call = late_step() if (f["retry"] and rng.random() < 0.5) else ("set_step", float(pick((1.0, 0.5, 0.25))), omega(), int(model.k))
        elif name == "set_omega":
            call = ("set_omega", omega())
        elif name == "set_iterate":
            call = ("set_iterate", int(rng.integers(100)))
        elif name == "flush_average":
            call = ("flush_average", ct.mode == "adaptive")
        elif name == "detect_infeasibility":
            call = ("detect_infeasibility", 1e-3)
        elif name == "spmv":
            call = ("spmv", int(rng.integers(100)), bool(rng.random() < 0.5))
        elif name == "power_iteration":
            call = ("power_iteration", int(rng.integers(100)), int(pick((1, 3, 6))))
        elif name == "set_option":
            call = ("set_option", pick(("RUNNING_KKT", "KTY_REUSE")), int(rng.integers(2)))
        elif name == "refused":
            call = ("refused", pick(("flush_average", "compute_average")))
        else:
            call = (name,)
        emit(call)
        count += name in CALLS
    return calls


# ---------------------------------------------------------------------------------------------------------------------
# hand-written sequences, one per transition of the engine's flags (names: what a failure points at)
# ---------------------------------------------------------------------------------------------------------------------
_S = [("set_iterate", 1), ("set_step", 1.0, 1.25, 0)]
_CHECK = lambda adaptive: [("kkt", CUR, 1.25, False), ("flush_average", adaptive), ("compute_average",), ("kkt", AVG, 1.25, False)]
_BYSTANDERS = [("report", CUR, False, 1.0), ("detect_infeasibility", 1e-3), ("spmv", 3, False), ("spmv", 4, True),
               ("power_iteration", 5, 3), ("report", PREV, True, 1.0), ("get_iterate", PREV)]
DIRECTED = {
    "kty_reuse": _S + [("iterate", 3, False), ("kkt", CUR, 1.25, False), ("iterate", 2, False), ("kkt", CUR, 1.25, False),
                       ("kkt", PREV, 1.25, False)],
    "kty_reuse_adaptive": _S + [("iterate", 3, True), ("kkt", CUR, 1.25, False), ("iterate", 1, True), ("kkt", CUR, 1.25, False),
                                ("iterate", 2, True), ("kkt", CUR, 0.75, False)],
    "kty_reuse_unscaled": _S + [("iterate", 2, False), ("kkt", CUR, 1.25, True), ("iterate", 3, False), ("kkt", CUR, 1.25, True),
                                ("kkt", CUR, 1.25, False)],
    "restart_cur_cached_kx": _S + [("iterate", 3, True), ("kkt", CUR, 1.25, False), ("restart", CUR), ("iterate", 2, True),
                                   ("kkt", CUR, 1.25, False)] + _CHECK(True),
    "restart_cur_swapped_kx": _S + [("kkt", CUR, 1.25, False), ("restart", CUR), ("iterate", 2, True), ("kkt", CUR, 1.25, False)]
    + _CHECK(True),
    "restart_cur_swapped_kx_fixed": [("set_iterate", 2), ("set_step", 1.0, 0.75, 0), ("iterate", 2, False), ("set_iterate", 3),
                                     ("kkt", CUR, 0.75, False), ("restart", CUR), ("iterate", 3, False)] + _CHECK(False),
    "flush_without_kkt_fixed": _S + [("iterate", 5, False), ("flush_average", False), ("compute_average",), ("kkt", AVG, 1.25, False),
                                     ("kkt", CUR, 1.25, False), ("restart", AVG), ("iterate", 2, False), ("kkt", CUR, 1.25, False)],
    "flush_without_kkt_adaptive": _S + [("iterate", 5, True), ("flush_average", True), ("compute_average",), ("kkt", AVG, 1.25, False),
                                        ("kkt", CUR, 1.25, False), ("iterate", 3, True)] + _CHECK(True)
    + [("restart", AVG), ("iterate", 2, True), ("kkt", CUR, 1.25, False)],
    "stale_average": _S + [("iterate", 3, False)] + _CHECK(False) + [("iterate", 2, False), ("kkt", AVG, 1.25, False),
                                                                     ("kkt", CUR, 1.25, False)],
    "stale_average_adaptive": _S + [("iterate", 5, True)] + _CHECK(True) + [("iterate", 3, True), ("kkt", AVG, 0.75, True),
                                                                           ("kkt", PREV, 1.25, False)],
    "second_check_fixed": _S + [("iterate", 3, False)] + _CHECK(False) + [("iterate", 2, False), ("kkt", AVG, 1.25, False)]
    + _CHECK(False) + [("restart", AVG), ("iterate", 1, False), ("kkt", CUR, 1.25, False)],
    "second_check_adaptive": _S + [("iterate", 3, True)] + _CHECK(True) + [("iterate", 2, True)] + _CHECK(True)
    + [("restart", AVG), ("iterate", 1, True), ("kkt", CUR, 1.25, False)],
    "second_check_same_iterate": _S + [("iterate", 5, True)] + _CHECK(True) + _CHECK(True) + [("flush_average", True),
                                                                                             ("compute_average",),
                                                                                             ("kkt", AVG, 1.25, False)],
    "adopted_average_overwritten": _S + [("iterate", 5, False)] + _CHECK(False) + [("restart", AVG), ("kkt", AVG, 1.25, False),
                                                                                   ("iterate", 2, False), ("kkt", CUR, 1.25, False)],
    "adopted_average_overwritten_adaptive": _S + [("iterate", 3, True)] + _CHECK(True) + [("restart", AVG), ("mark_restart_point",),
                                                                                          ("kkt", AVG, 1.25, True), ("iterate", 3, True),
                                                                                          ("kkt", CUR, 1.25, False)],
    "adopted_average_overwritten_then_cur": _S + [("iterate", 8, False)] + _CHECK(False) + [("restart", AVG), ("kkt", AVG, 1.25, False),
                                                                                            ("kkt", CUR, 1.25, False), ("iterate", 1, False),
                                                                                            ("kkt", CUR, 1.25, False)],
    "restart_avg_without_kkt": _S + [("iterate", 5, True), ("kkt", CUR, 1.25, False), ("flush_average", True), ("compute_average",),
                                     ("restart", AVG), ("restart_distance",), ("mark_restart_point",), ("iterate", 3, True),
                                     ("kkt", CUR, 1.25, False)] + _CHECK(True),
    "restart_avg_without_kkt_fixed": _S + [("iterate", 3, False), ("flush_average", False), ("compute_average",), ("restart", AVG),
                                           ("iterate", 2, False), ("kkt", CUR, 1.25, False)] + _CHECK(False),
    "double_restart": _S + [("iterate", 3, True)] + _CHECK(True) + [("restart", AVG), ("restart", CUR), ("iterate", 2, True),
                                                                   ("kkt", CUR, 1.25, False), ("restart", CUR), ("restart", CUR),
                                                                   ("iterate", 1, True), ("kkt", CUR, 1.25, False)],
    "double_restart_fixed": _S + [("iterate", 2, False), ("kkt", CUR, 1.25, False), ("restart", CUR), ("restart", CUR),
                                  ("iterate", 3, False)] + _CHECK(False) + [("restart", AVG), ("restart", CUR), ("iterate", 2, False),
                                                                           ("kkt", CUR, 1.25, False)],
    # (8 x the safe step late in a solve: the first trial is accepted with eta' next to eta_bar, the trials after it are rejected --
    # test_sequences_host.py checks that every retry here follows a rejected trial)
    "retry_then_check": [("set_iterate", 1), ("set_step", 8.0, 1.25, 100000), ("iterate", 1, True), ("iterate", 1, True), ("adaptive_retry",),
                         ("iterate", 1, True), ("adaptive_retry",), ("iterate", 3, True)] + _CHECK(True)
    + [("kkt", PREV, 1.25, False), ("restart", AVG), ("iterate", 2, True), ("kkt", CUR, 1.25, False)],
    "retry_after_check": [("set_iterate", 4), ("set_step", 1.0, 1.25, 0), ("iterate", 3, True)] + _CHECK(True)
    + [("restart", AVG), ("set_step", 8.0, 1.25, 100000), ("iterate", 1, True), ("iterate", 1, True), ("adaptive_retry",),
       ("kkt", CUR, 1.25, False), ("iterate", 2, True)] + _CHECK(True),
    "retry_mid_period": [("set_iterate", 5), ("set_step", 8.0, 0.75, 100000), ("iterate", 1, True), ("iterate", 1, True),
                         ("kkt", CUR, 0.75, False), ("adaptive_retry",), ("iterate", 2, True), ("kkt", CUR, 0.75, False),
                         ("flush_average", True), ("compute_average",), ("kkt", AVG, 0.75, False), ("get_iterate", AVG)],
    "halpern_then_pdhg": _S + [("halpern_iterate", 5), ("kkt", AVG, 1.25, False), ("refused", "flush_average"),
                               ("refused", "compute_average"), ("restart", AVG), ("mark_restart_point",), ("iterate", 3, False),
                               ("kkt", CUR, 1.25, False), ("kkt", PREV, 1.25, False)],
    "halpern_then_pdhg_adaptive": _S + [("halpern_iterate", 3), ("kkt", CUR, 1.25, False), ("kkt", AVG, 1.25, True), ("restart", AVG),
                                        ("restart_distance",), ("mark_restart_point",), ("iterate", 2, True), ("kkt", CUR, 1.25, False),
                                        ("halpern_iterate", 2), ("kkt", AVG, 1.25, False)],
    "halpern_restart_cur": _S + [("halpern_iterate", 2), ("kkt", CUR, 1.25, False), ("restart", CUR), ("mark_restart_point",),
                                 ("halpern_iterate", 3), ("kkt", AVG, 1.25, False), ("restart", AVG), ("mark_restart_point",),
                                 ("iterate", 1, False), ("kkt", CUR, 1.25, False)],
    "pdhg_then_halpern": _S + [("iterate", 5, False)] + _CHECK(False) + [("restart", AVG), ("mark_restart_point",), ("halpern_iterate", 3),
                                                                        ("kkt", AVG, 1.25, False), ("kkt", CUR, 1.25, False),
                                                                        ("restart", AVG), ("halpern_iterate", 1), ("get_iterate", AVG)],
    "pdhg_then_halpern_adaptive": _S + [("iterate", 3, True), ("kkt", CUR, 1.25, False), ("restart", CUR), ("halpern_iterate", 2),
                                        ("kkt", AVG, 1.25, False), ("report", AVG, False, 1.0), ("halpern_iterate", 2),
                                        ("kkt", AVG, 1.25, False)],
    "pdhg_then_halpern_kept_kty": _S + [("iterate", 2, False), ("kkt", CUR, 1.25, False), ("halpern_iterate", 1), ("kkt", AVG, 1.25, False),
                                        ("restart", AVG), ("mark_restart_point",), ("halpern_iterate", 2), ("kkt", AVG, 1.25, False)],
    "options_toggled": _S + [("iterate", 3, False), ("set_option", "RUNNING_KKT", 0)] + _CHECK(False)
    + [("set_option", "RUNNING_KKT", 1), ("iterate", 2, False)] + _CHECK(False) + [("set_option", "KTY_REUSE", 0), ("iterate", 1, False),
                                                                                 ("kkt", CUR, 1.25, False), ("set_option", "KTY_REUSE", 1),
                                                                                 ("iterate", 1, False), ("kkt", CUR, 1.25, False)],
    "options_toggled_adaptive": _S + [("iterate", 3, True), ("kkt", CUR, 1.25, False), ("set_option", "KTY_REUSE", 0), ("iterate", 2, True),
                                      ("set_option", "RUNNING_KKT", 0), ("kkt", CUR, 1.25, False), ("set_option", "RUNNING_KKT", 1),
                                      ("flush_average", True), ("compute_average",), ("kkt", AVG, 1.25, False), ("restart", AVG),
                                      ("set_option", "KTY_REUSE", 1), ("iterate", 2, True), ("kkt", CUR, 1.25, False)],
    "options_toggled_before_restart": _S + [("iterate", 5, False)] + _CHECK(False) + [("set_option", "RUNNING_KKT", 0), ("restart", AVG),
                                                                                     ("iterate", 2, False), ("kkt", CUR, 1.25, False),
                                                                                     ("set_option", "RUNNING_KKT", 1)] + _CHECK(False),
    # graph replay on for part of a period (the running sums are not kept under replay), off again before the check
    "options_toggled_graph": _S + [("iterate", 2, False), ("set_option", "GRAPH", 1), ("iterate", 8, False), ("set_option", "GRAPH", 0),
                                   ("iterate", 2, False)] + _CHECK(False) + [("restart", AVG), ("iterate", 2, False),
                                                                             ("kkt", CUR, 1.25, False)],
    # graph replay from the first iteration of a period, an even count (replays only), off again, direct iterations, a check: the
    # period has run eight iterations, the running product sums would hold the last two (a replay has to count as iterations)
    "graph_even_replays_from_restart": _S + [("iterate", 2, False), ("kkt", CUR, 1.25, False), ("restart", CUR), ("set_option", "GRAPH", 1),
                                             ("iterate", 6, False), ("set_option", "GRAPH", 0), ("iterate", 2, False)] + _CHECK(False)
    + [("restart", AVG), ("iterate", 2, False), ("kkt", CUR, 1.25, False)],
    # eta changes INSIDE a fixed-step period: K'y of an iterate used to join its running sum with the eta of the NEXT iteration
    # while y_sum had it with its own, so K'y_avg from the sums was not K' y_avg (pdlp_set_step now ends the running sums)
    "set_step_mid_period": _S + [("iterate", 3, False), ("set_step", 0.5, 1.25, 3), ("iterate", 2, False)] + _CHECK(False)
    + [("restart", AVG), ("iterate", 2, False), ("kkt", CUR, 1.25, False)],
    "set_step_mid_period_longer": _S + [("iterate", 1, False), ("set_step", 2.0, 1.25, 1), ("iterate", 1, False),
                                        ("set_step", 0.5, 1.25, 2), ("iterate", 3, False)] + _CHECK(False)
    + [("restart", AVG), ("iterate", 1, False), ("kkt", CUR, 1.25, False)],
    "set_step_mid_period_adaptive": _S + [("iterate", 3, True), ("set_step", 0.5, 0.75, 3), ("iterate", 2, True),
                                          ("kkt", CUR, 0.75, False), ("flush_average", True), ("compute_average",),
                                          ("kkt", AVG, 0.75, False), ("restart", AVG), ("iterate", 2, True), ("kkt", CUR, 0.75, False)],
}
# the calls that must leave every later number alone, put between the calls of a check and after the restart that follows it
for _i, _b in enumerate(_BYSTANDERS):
    _ad = bool(_i % 2)
    _seq = _S + [("iterate", 3, _ad)]
    for _c in _CHECK(_ad):
        _seq = _seq + [_c, _b]
    _after = _b if _b[0] in ("spmv", "power_iteration") else ("report", CUR, True, 1.0)        # (PREV is gone after a restart)
    DIRECTED[f"bystander_{_i}_{_b[0]}"] = _seq + [("iterate", 2, _ad), _b, ("kkt", CUR, 1.25, False), ("restart", AVG), _after,
                                                  ("iterate", 1, _ad), ("kkt", CUR, 1.25, False)]


def restricted(calls, features):
    """whether a directed sequence fits a configuration's grammar"""
    f = dict(FULL, **features)
    for c in calls:
        if (c[0] == "adaptive_retry" and not f["retry"]) or (c[0] == "halpern_iterate" and not f["halpern"]):
            return False
        if c[0] in ("iterate", "flush_average") and c[-1] and not f["adaptive"]:
            return False
        if c[:2] == ("set_option", "GRAPH") and not f["graph_toggle"]:
            return False
        if f["delta"] and c[0] == "kkt" and c[1] != CUR and c[3]:       # (delta mode un-scales at the current iterate only)
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------------
# the situations of DIRECTED, recognised in any list of calls (for the coverage counts)
# ---------------------------------------------------------------------------------------------------------------------
def situations(calls):
    """Counter of the flag transitions a sequence walks through, told from the calls alone by following what a handle that carries
    its products would have at hand (not what the engine's code does: what the header's description of the savings implies)"""
    out = Counter()
    kx_carried = False               # K x of the current x is carried along (an iteration has run since the last reset of it)
    kkt_cur = None                   # a KKT pass at the CURRENT iterate is still fresh: (unscaled, K x was carried)
    mode, its, flushed, flushes, averaged, moved_since_avg = None, 0, False, 0, False, False
    adopted_from_sums = restarted = retried = bystander = False
    last_period = None
    for c in calls:
        name = c[0]
        if name in ("report", "detect_infeasibility", "spmv", "power_iteration"):
            bystander = True
            continue
        if name in ("get_iterate", "restart_distance", "mark_restart_point", "infeas_reset", "set_omega", "refused", "refresh_products"):
            continue
        if name == "set_option":
            out["option_toggled"] += 1
            continue
        if name == "set_step":
            if its > 0 and mode in ("fixed", "adaptive"):
                out["set_step_mid_period"] += 1
            continue
        if name == "iterate":
            if kkt_cur is not None:
                out["kty_reuse_unscaled" if kkt_cur[0] else "kty_reuse"] += 1
            if restarted and kkt_cur is None and last_period == "halpern":
                out["halpern_then_pdhg"] += 1
            if restarted and restarted != "plain":
                out[restarted] += 1
            if bystander:
                out["bystander_then_iterate"] += 1
            mode, its = ("adaptive" if c[2] else "fixed"), its + c[1]
            kx_carried, kkt_cur, flushed, moved_since_avg = True, None, False, averaged
            restarted = adopted_from_sums = bystander = False
        elif name == "halpern_iterate":
            if last_period in ("fixed", "adaptive") and mode is None:
                out["pdhg_then_halpern"] += 1
            mode, its, kx_carried, kkt_cur, averaged = "halpern", its + c[1], False, None, False
            restarted = adopted_from_sums = bystander = False
        elif name == "adaptive_retry":
            its, kx_carried, kkt_cur, retried, flushed = its - 1, False, None, True, False
        elif name == "kkt":
            if c[1] == CUR:
                kkt_cur = (bool(c[3]), kx_carried)
                if adopted_from_sums:
                    adopted_from_sums = False
            elif c[1] == AVG:
                if adopted_from_sums:
                    out["adopted_average_overwritten"] += 1
                    adopted_from_sums = False
                elif averaged and moved_since_avg:
                    out["stale_average"] += 1
                elif averaged and flushes >= 2 and mode != "halpern":
                    out["second_check"] += 1
                if averaged and retried:
                    out["retry_then_check"] += 1
                if averaged and mode != "halpern":
                    averaged = "checked"
        elif name == "flush_average":
            if kkt_cur is None and its > 0:
                out["flush_without_kkt_" + ("adaptive" if c[1] else "fixed")] += 1
            flushed, flushes = True, flushes + 1
        elif name == "compute_average":
            averaged, moved_since_avg = True, False
        elif name in ("restart", "set_iterate"):
            if name == "restart":
                if restarted:
                    out["double_restart"] += 1
                if c[1] == CUR:
                    restarted = "plain" if kkt_cur is None else ("restart_cur_cached_kx" if kkt_cur[1] else "restart_cur_swapped_kx")
                else:
                    restarted = "restart_avg_without_kkt" if (averaged is True and mode != "halpern") else "plain"
                    adopted_from_sums = averaged == "checked"
                    kx_carried = averaged == "checked" or mode == "halpern"
                last_period = mode
            else:
                restarted, last_period, kx_carried, adopted_from_sums = False, None, False, False
            kkt_cur = None if (name == "set_iterate" or c[1] == AVG) else kkt_cur
            mode, its, flushed, flushes, averaged, moved_since_avg, retried = None, 0, False, 0, False, False, False
    return out


SITUATIONS = ("kty_reuse", "kty_reuse_unscaled", "restart_cur_cached_kx", "restart_cur_swapped_kx", "flush_without_kkt_fixed",
              "flush_without_kkt_adaptive", "stale_average", "second_check", "adopted_average_overwritten", "restart_avg_without_kkt",
              "double_restart", "retry_then_check", "bystander_then_iterate", "halpern_then_pdhg", "pdhg_then_halpern", "option_toggled",
              "set_step_mid_period")
SEEDS = tuple(range(40))             # the committed seed set of the random sequences
