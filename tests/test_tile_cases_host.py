"""The constructed matrices of tests/tile_cases.py on the CPU: every case really sits on the edge it is named after (its predicates
hold on the built tiles), the tiles respect what the kernel trusts without checking, and the torch replay of the kernel's two passes
gives the exact product within 1e-11 of the largest row's sum |K||v| (the replay takes a row's sum as a difference of two running
sums over its tile, so its own rounding is relative to the tile's sum, not the row's; the per-row bound is the GPU test's).  A failing predicate is a broken case: nothing here skips.  (The GPU side: tests/test_gpu_tile_edges.py.)"""
import numpy as np
import pytest

from tests import handle_model as hm
from tests import tile_cases as tc
from torchpdlp_amd.tiled import emulate_spmv, normalize_groups

import torch

CASE_PREC = [(n, p) for n in tc.NAMES for p in tc.LIMITS]


def test_limits_table():
    from torchpdlp_amd import tiled as T
    assert tc.LIMITS["f32"][:2] == (T.RPT_MAX, T.CAP) == T.limits(torch.float32) and tc.LIMITS["f64"][:2] == T.limits(torch.float64)
    assert tc.LIMITS["mixed"][:2] == tc.LIMITS["f32"][:2]                       # one float32 tile set serves both kernels
    for lim, tu in zip(tc.LIMITS.values(), (4, 2, 2)):
        assert lim.group == lim.nt * 4 * tu and lim.cap % lim.group == 0 and lim.nt == T.NT


@pytest.mark.parametrize("name,prec", CASE_PREC)
def test_case_holds_its_edge(name, prec):
    case, lim = tc.get_case(name, prec), tc.LIMITS[prec]
    assert np.array_equal(case.A.data, case.A.data.astype(np.float32).astype(np.float64)) and case.A.has_sorted_indices
    v = tc.probe(case.A.shape[1])
    ref, mag, items = tc.exact_product(case.A, v)
    x = torch.from_numpy(v).to(tc.VALUE_DTYPE[prec])
    for groups in case.groups:
        t = tc.build(case, prec, groups)
        assert t is not None, "the case matrix must be tiled"
        assert t.groups == groups
        assert tc.format_violations(t, lim) == []
        for what, holds in case.predicates:
            assert holds(t), f"{name} [{prec}] does not hold its edge: {what}"
        if groups == case.groups[0]:
            assert t.stats["tiled"] + t.nrem == case.A.nnz and int(tc.real_sizes(t).sum()) == t.stats["tiled"]
            got = emulate_spmv(t, x).numpy()
            assert np.abs(got - ref).max() <= 1e-11 * mag.max(), float(np.abs(got - ref).max())
            assert np.all(got[items == 0] == 0)


@pytest.mark.parametrize("name,prec", CASE_PREC)
def test_transposed_case(name, prec):
    """the other side of an engine around the case: tiled with the same explicit arguments, or left to the CSR kernel"""
    case, lim = tc.get_case(name, prec), tc.LIMITS[prec]
    t = tc.build(case, prec, 1, transposed=True)
    assert (t is None) == case.other_side_csr
    if t is None:
        return
    assert tc.format_violations(t, lim) == []
    AT = case.A.T.tocsr()
    v = tc.probe(AT.shape[1], 6)
    ref, mag, _ = tc.exact_product(AT, v)
    got = emulate_spmv(t, torch.from_numpy(v).to(tc.VALUE_DTYPE[prec])).numpy()
    assert np.abs(got - ref).max() <= 1e-11 * mag.max()


def test_group_counts_the_builder_folds():
    """9 panels in 4 or 8 groups: the builder's rule gives 3 and 5, the case sets the count the library is handed"""
    assert [normalize_groups(g, 9, 32) for g in (4, 5, 8, 9)] == [3, 5, 5, 9]
    assert [normalize_groups(g, 5, 32) for g in (1, 2, 3, 5)] == [1, 2, 3, 5] and [normalize_groups(g, 3, 32) for g in (1, 2, 3)] == [1, 2, 3]
    # k_rowsum_epilogue adds four groups per round trip: a count that is no multiple of four re-reads the clamped last group
    assert sorted(g % 4 for g in tc.get_case("many_groups", "f32").groups) == [0, 0, 1, 1, 1]


def test_a_malformed_tile_set_is_reported():
    """the check that stands between a tile set and ``attach_tiles`` does see a broken one"""
    case = tc.get_case("counts", "f32")
    t = tc.build(case, "f32")
    assert tc.format_violations(t, tc.LIMITS["f32"]) == [] and tc.format_violations(t, tc.LIMITS["f64"]) != []
    t.cnt = t.cnt.clone()
    t.cnt[0] = 0x44444444 | t.cnt[0]                     # a run of 255 grows
    assert any("64 consecutive rows" in s for s in tc.format_violations(t, tc.LIMITS["f32"]))


@pytest.mark.parametrize("side", ["K", "KT"])
@pytest.mark.parametrize("name,prec", CASE_PREC)
def test_adaptive_step_of_the_sequence_is_decided(name, prec, side):
    """the epilogue check walks one adaptive step: the model must accept or reject it by a margin no rounding of a float32 engine
    reaches, |eta - eta_bar| / eta_bar > 1e-2"""
    lp = tc.get_lp(name, prec, side)
    assert lp.m_ineq == 2 * lp.m // 5 and (lp.n < 4 or (np.isinf(lp.l).any() and np.isinf(lp.u).any() and (lp.l == lp.u).any()))
    model = hm.HandleModel(lp)
    for call in tc.SEQUENCE:
        if call[0] == "iterate" and call[2]:
            eta = model.eta
            _, _, _, _, info = model.o.step_adaptive(model.x, model.y, model.eta, model.omega, model.theta, model.k + 1)
            margin = abs(eta - info["eta_bar"]) / info["eta_bar"]
            assert margin > 1e-2, (margin, eta, info)
        model.apply(call)
    assert model.k == 2 and model.xp is not None
