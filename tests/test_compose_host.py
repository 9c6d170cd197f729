"""The composition rule of the three problem-class switches (torchpdlp_amd/compose.py) on the host: every switch against every
form it does not have, through all four entry points with the same message, and every combination the docstrings list as working.
No device: solve_lp / pdlp_algorithm refuse before any device work, the driver before it uses the engine."""
import itertools
from types import SimpleNamespace

import pytest
import torch

import torchpdlp_amd as tp
from tests.test_halpern_fixed_point_host import Untouchable
from torchpdlp_amd import batch, compose, quad, ranged, solver
from torchpdlp_amd.engine import PdlpEngine
from torchpdlp_amd.solver import PdhgDriver, pdlp_algorithm

INF = float("inf")
K3, V3 = torch.eye(3), torch.zeros(3)
QU, D3 = torch.tensor([1.0, INF, INF]), torch.ones(3)
MESSAGE = dict(halpern=compose.HALPERN_REFUSED, q_upper=compose.RANGED_REFUSED, quad_diag=compose.QUAD_REFUSED)
SWITCH_KW = dict(halpern=dict(halpern=True), q_upper=dict(q_upper=QU), quad_diag=dict(quad_diag=D3))
# the refused conditions, as compose.check_composition names them; `adaptive` is refused by the Halpern mode only, `fishnet` by the
# two problem classes only
CONDITIONS = ("adaptive", "adaptive_retry", "infeasibility_detect", "mixed", "comm", "fishnet", "direct_exchange")
REFUSED = [(s, c) for s in MESSAGE for c in CONDITIONS if not (c == "adaptive" and s != "halpern") and not (c == "fishnet" and s == "halpern")]


def raises(message, fn, *a, **kw):
    with pytest.raises(ValueError) as e:
        fn(*a, **kw)
    assert str(e.value) == message


def as_keywords(cond, names):
    """the condition as keyword arguments of solve_lp / pdlp_algorithm (None: the entry point has no such argument)"""
    if cond == "mixed":
        return dict(precision="mixed")
    if cond == "comm":
        return dict(comm=True)
    if cond == "adaptive_retry":                     # (the flag of the adaptive step)
        return {names.get("adaptive", "adaptive"): True, "adaptive_retry": True}
    if cond in ("fishnet", "direct_exchange") and not names:
        return None
    return {names.get(cond, cond): True}


class Engine(Untouchable):
    """the host tests' untouchable engine with what PdhgDriver reads of the two problem classes before it refuses"""
    q_upper, quad_diag = None, None

    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_the_constants_are_importable_under_their_old_names():
    assert ranged.REFUSED is compose.RANGED_REFUSED and quad.REFUSED is compose.QUAD_REFUSED
    assert solver.HALPERN_REFUSED is compose.HALPERN_REFUSED
    assert "adaptive" in batch.HALPERN_BATCH_REFUSED
    assert len({compose.HALPERN_REFUSED, compose.RANGED_REFUSED, compose.QUAD_REFUSED}) == 3


@pytest.mark.parametrize("switch,cond", REFUSED, ids=lambda v: v)
def test_each_switch_against_each_refused_condition(switch, cond):
    msg = MESSAGE[switch]
    raises(msg, compose.check_composition, **{switch: True, cond: True})
    # solve_lp knows every condition
    kw = as_keywords(cond, dict(adaptive="adaptive_stepsize"))
    raises(msg, tp.solve_lp, (V3, K3, V3, 2, V3, V3 + 1), device="cpu", **SWITCH_KW[switch], **kw)
    # pdlp_algorithm has no fishnet / direct_exchange
    kw = as_keywords(cond, {})
    if kw is not None:
        raises(msg, pdlp_algorithm, K3, 2, V3, V3, V3, V3 + 1, "cpu", verbose=False, **SWITCH_KW[switch], **kw)
    # the driver reads mixed and comm off the engine, and the two problem classes too
    if cond not in ("fishnet", "direct_exchange"):
        eng = Engine(q_upper=QU if switch == "q_upper" else None, quad_diag=D3 if switch == "quad_diag" else None,
                     mixed=cond == "mixed", comm=SimpleNamespace(world=2) if cond == "comm" else None)
        dkw = {} if cond in ("mixed", "comm") else as_keywords(cond, {})
        raises(msg, PdhgDriver, eng, halpern=switch == "halpern", **dkw)
    # PdlpEngine.set_row_upper: what an engine can be
    if switch == "q_upper" and cond in ("mixed", "comm"):
        eng = SimpleNamespace(mixed=cond == "mixed", comm=object() if cond == "comm" else None)
        raises(msg, PdlpEngine.set_row_upper, eng, QU)


def test_two_refusals_at_once_come_in_one_order_everywhere():
    """Halpern, then q_upper, then quad_diag"""
    for kw, msg in ((dict(halpern=True, q_upper=True, quad_diag=True), compose.HALPERN_REFUSED),
                    (dict(q_upper=True, quad_diag=True), compose.RANGED_REFUSED), (dict(quad_diag=True), compose.QUAD_REFUSED)):
        raises(msg, compose.check_composition, infeasibility_detect=True, **kw)
    both = dict(halpern=True, q_upper=QU, infeasibility_detect=True)
    raises(compose.HALPERN_REFUSED, tp.solve_lp, (V3, K3, V3, 2, V3, V3 + 1), device="cpu", **both)
    raises(compose.HALPERN_REFUSED, pdlp_algorithm, K3, 2, V3, V3, V3, V3 + 1, "cpu", verbose=False, **both)
    raises(compose.HALPERN_REFUSED, PdhgDriver, Engine(q_upper=QU), halpern=True, infeasibility_detect=True)


def test_every_combination_the_docstrings_list_as_working_passes():
    """the three switches in every combination with each other, with and without the adaptive step where the Halpern mode is off
    (precondition, primal_update, pock_chambolle and the start vectors are no inputs of the rule), Halpern behind a fishnet start"""
    for h, r, d in itertools.product((False, True), repeat=3):
        compose.check_composition(halpern=h, q_upper=r, quad_diag=d)
        if not h:
            compose.check_composition(q_upper=r, quad_diag=d, adaptive=True)
    compose.check_composition(halpern=True, fishnet=True)
    # with no switch on, nothing is refused here
    compose.check_composition(**{c: True for c in CONDITIONS})


def test_malformed_vectors_are_still_reported_before_any_device_work():
    raises("quad_diag holds a negative entry (the objective must stay convex: d >= 0)", tp.solve_lp, (V3, K3, V3, 2, V3, V3 + 1),
           device="cpu", quad_diag=-D3)
    with pytest.raises(ValueError, match="q_upper"):
        pdlp_algorithm(K3, 2, V3, V3, V3, V3 + 1, "cpu", verbose=False, q_upper=torch.tensor([-1.0, INF, INF]))
