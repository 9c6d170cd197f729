"""The float64 model of the handle and the call sequences of tests/handle_model.py, checked on the host (no GPU): the model against
the float64 oracle's whole solves, what the committed sequences cover, and how far a stale product would be from the right one."""
from collections import Counter

import numpy as np
import pytest

from oracle import oracle as orc
from tests import handle_model as hm
from tests.conftest import Golden
from tests.host_lp import HostLP, get_lp
from torchpdlp_amd import rules

F64 = np.float64


def _golden_lp(name):
    a = Golden("solve_trace.npz").group(name)
    import scipy.sparse as sp
    A = sp.csr_matrix((a["val"], a["colidx"], a["rowptr"]), shape=(int(a["m"]), int(a["n"])))
    return HostLP(A, int(a["m_ineq"]), a["c"], a["q"], a["l"], a["u"])


def solve_with_model(lp, adaptive, sigma, tol, max_kkt, restart_period=40):
    """the solver's own order of calls (PdhgDriver, solver.py; pdhg.py:54-176) on the model: iterate -> kkt(CUR) -> flush -> average ->
    kkt(AVG) -> kkt(PREV) -> restart -> restart_distance -> set_omega -> mark -> kkt(CUR)"""
    m = hm.HandleModel(lp)
    q_norm, c_norm = F64(np.sqrt(np.sum(lp.q ** 2))), F64(np.sqrt(np.sum(lp.c ** 2)))
    omega = rules.start_omega(q_norm, c_norm, F64)
    m.set_iterate(np.zeros(lp.n), np.zeros(lp.m))
    m.set_step(rules.start_eta(sigma, F64), omega, 1.0, 0)
    kkt_first, j, n_out, status, trace = F64(0), 0, 0, rules.STATUS_KKT_LIMIT, []
    while j < max_kkt:
        tt = 0
        m.mark_restart_point()
        while j < max_kkt:
            steps = min(restart_period, max_kkt - j)
            m.iterate(steps, adaptive)
            j, tt = j + steps, tt + steps
            if tt % restart_period:
                break
            r_cur = m.kkt(hm.CUR, omega)
            m.flush_average(adaptive)
            m.compute_average()
            r_avg, r_prev = m.kkt(hm.AVG, omega), m.kkt(hm.PREV, omega)
            trace += [r_cur["kkt"], r_avg["kkt"], r_prev["kkt"]]
            j += 3
            d = rules.restart_decision(r_cur["kkt"], r_avg["kkt"], r_prev["kkt"], kkt_first, tt, m.k, j, t=F64)
            if d["crit"] >= 0:
                m.restart(hm.AVG if d["use_avg"] else hm.CUR)
                break
        n_out += 1
        # the new primal weight by the oracle's own routine (rules.primal_weight agrees with it to an ulp of its log and exp, which 40
        # adaptive steps amplify 10^4-fold); the model's two distances are what that routine starts from
        dx2, dy2 = m.restart_distance()
        assert (dx2, dy2) == (float(np.sum((m.x - m.x_last) ** 2)), float(np.sum((m.y - m.y_last) ** 2)))
        np.testing.assert_allclose(rules.primal_weight(dx2, dy2, omega, 0.5, F64), m.o.primal_weight(m.x_last, m.x, m.y_last, m.y, omega), rtol=1e-14)
        omega = m.o.primal_weight(m.x_last, m.x, m.y_last, m.y, omega, 0.5)
        m.set_omega(omega)
        res = m.kkt(hm.CUR, omega)
        kkt_first = F64(res["kkt"])
        trace.append(res["kkt"])
        j += 2
        if rules.terminated(res, q_norm, c_norm, tol, F64):
            status = rules.STATUS_SOLVED
            break
    return m, n_out, j, status, trace


@pytest.mark.parametrize("adaptive", [False, True], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("name", ["mixed_27x32", "mixed_400x300"])
def test_model_in_the_solvers_order_is_the_float64_oracle(name, adaptive):
    """guards the model itself: driven in the project's own order, with the restart rule of rules.py and the primal weight update,
    it reproduces the float64 ``oracle.pdlp_algorithm`` run of the same LP -- iteration, restart and KKT-pass counts, every KKT
    error of every check and the final x to 1e-12 relative (the pass count is capped: the agreement does not need a whole solve)"""
    orc.set_threads(1)
    lp = _golden_lp(name)
    o = lp.oracle(F64)
    sigma = o.power_iter(np.ones(lp.n), 60)
    x, _, k, n_out, j, status, _, tr = orc.pdlp_algorithm(o, max_kkt=1500, tol=1e-7, primal_update=True, adaptive=adaptive, sigma=sigma)
    m, n_model, j_model, status_model, trace = solve_with_model(lp, adaptive, sigma, 1e-7, 1500)
    assert (m.k, n_model, j_model, status_model) == (k, n_out, j, status)
    assert n_out >= 3 and any(use_avg for _, _, use_avg in tr["restarts"])           # (restarts to the average happened)
    np.testing.assert_allclose(trace, tr["kkt"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(m.x, x, rtol=1e-12, atol=1e-12 * np.abs(x).max())


def _all_sequences(lp):
    """name -> (calls, the model after them): the 40 random sequences of the full grammar and the directed list"""
    out = {}
    for seed in hm.SEEDS:
        model = hm.HandleModel(lp)
        out[f"seed{seed}"] = (hm.generate(lp, seed, model=model), model)
    for name, calls in hm.DIRECTED.items():
        model = hm.HandleModel(lp)
        for c in calls:
            model.apply(c)
        out[name] = (calls, model)
    return out


@pytest.fixture(scope="module", params=["seq", "mid_scaled"])
def sequences(request):
    orc.set_threads(1)
    return _all_sequences(get_lp(request.param))


def test_random_sequences_keep_to_the_grammar(sequences):
    lp = next(iter(sequences.values()))[1].lp
    for name, (calls, _) in sequences.items():
        if not name.startswith("seed"):
            continue
        assert calls[0][0] == "set_iterate" and calls[1][0] == "set_step", name
        assert 22 <= sum(c[0] in hm.CALLS for c in calls) <= 30, name
        assert calls == hm.generate(lp, int(name[4:])), name                     # (a seed names a sequence)
        ct = hm.Contract()
        model = hm.HandleModel(lp)
        for c in calls:
            if c[0] in ("kkt", "report", "get_iterate"):
                assert ct.defined(c[1]), (name, c)
            if c[0] == "restart":
                assert ct.defined(c[1]), (name, c)
            if c[0] == "detect_infeasibility":
                assert ct.prev, (name, c)
            if c[0] == "adaptive_retry":
                assert ct.retry_ok, (name, c)
            if c[0] in ("flush_average", "compute_average"):
                assert not ct.halpern_since_set and ct.weight, (name, c)
            if c[0] == "flush_average":
                assert c[1] == (ct.mode == "adaptive"), (name, c)
            if c[0] == "iterate" and ct.mode is not None:
                assert ct.mode == ("adaptive" if c[2] else "fixed"), (name, c)
            if c[0] == "halpern_iterate":
                assert ct.mode in (None, "halpern"), (name, c)
            if c[0] == "refused":
                assert ct.halpern_since_set, (name, c)
            if c[0] == "set_step":
                assert ct.its == 0, (name, c)
            if c[0] in ("iterate", "halpern_iterate"):
                assert c[1] in hm.ITERS, (name, c)
            model.apply(c)
            ct.after(c, rejected=c[0] == "iterate" and bool(c[2]) and not model.accepted)


def test_directed_retries_follow_rejected_trials(sequences):
    """the header allows pdlp_adaptive_retry after a REJECTED trial only: every retry of the directed list is one"""
    for name, (calls, _) in sequences.items():
        if name.startswith("seed"):
            continue
        model = hm.HandleModel(next(iter(sequences.values()))[1].lp)
        for prev, c in zip([None] + list(calls), calls):
            if c[0] == "adaptive_retry":
                assert prev[0] in ("iterate", "kkt") and not model.accepted, (name, prev)
            model.apply(c)


def test_coverage_of_the_committed_sequences(sequences):
    """counted from the calls alone, over the 40 seeds and the directed list: every call of the grammar at least 40 times, every
    situation of the directed list at least 3 times"""
    calls, seen = Counter(), Counter()
    for seq, _ in sequences.values():
        calls.update(c[0] for c in seq)
        seen.update(hm.situations(seq))
    assert len(hm.CALLS) == 18
    short = {c: calls[c] for c in hm.CALLS if calls[c] < 40}
    assert not short, short
    rare = {s: seen[s] for s in hm.SITUATIONS if seen[s] < 3}
    assert not rare, rare
    assert 25 <= len(hm.DIRECTED)


def test_a_stale_product_is_far_from_the_right_one(sequences):
    """the discrimination condition: at every iteration of every sequence K'y and K x of the new iterate differ from those of the
    previous one, and at every average (every Halpern candidate) those of the average from those of the current iterate, by at
    least 1e-4 relative to 1 + the product's size -- 10^4 float64 tolerances or more.  (Left out, because the two points coincide
    there by construction: the average after ONE iteration, and the first Halpern candidate from the anchor.)"""
    worst = {}
    for name, (_, model) in sequences.items():
        for what, v in model.margins:
            if v < worst.get(what, (np.inf, ""))[0]:
                worst[what] = (v, name)
    print(worst)
    assert set(worst) == {"kty", "kx", "kty_avg", "kx_avg"}
    assert all(v >= 1e-4 for v, _ in worst.values()), worst
