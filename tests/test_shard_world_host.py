"""What tests/test_gpu_shard_world.py relies on, checked without a GPU: the helper's restatement of the header's exchange contract
(tests/shard_world.py) against brute force, its padding and permutation against the unsharded float64 model, the robustness of the
adaptive decisions its runs take, and that the directed list of configurations really holds the cases it was chosen for."""
import numpy as np
import pytest

from tests import handle_model as hm
from tests import shard_world as sw

SHAPES = [(w, lw, ch) for w in sw.WORLDS for lw in sw.LWS for ch in (1, 2, 3, 4)]


def _blocks(world):
    lp = sw.world_lp()
    return -(-lp.n // world), -(-lp.m // world)


@pytest.mark.parametrize("B", [1, 63, 64, 127, 128, 191, 192, 255, 256, 257, 1006, 1600, 2011, 2681, 3200, 4021, 4267, 6400])
def test_plan_bounds_cover_the_block(B):
    """c*B/C rounded down to 64, one piece when B < 64*C: the pieces cover [0, B) without overlap, none is empty"""
    for chunks in (1, 2, 3, 4):
        b = sw.plan_bounds(B, chunks)
        C = chunks if B >= 64 * chunks else 1
        assert len(b) == C + 1 and b[0] == 0 and b[-1] == B
        assert all(lo < hi for lo, hi in zip(b[:-1], b[1:]))
        assert all(v % 64 == 0 and v == (c * B // C) // 64 * 64 for c, v in enumerate(b[:-1]))
        covered = np.zeros(B, np.int64)
        for lo, hi in zip(b[:-1], b[1:]):
            covered[lo:hi] += 1
        assert (covered == 1).all()


@pytest.mark.parametrize("world,lw,chunks", SHAPES)
def test_panel_ready_piece_against_arrival_simulation(world, lw, chunks):
    """every entry of the gathered vector gets the piece it travels in (-1: the rank's own block); a panel is ready with the last
    of its entries"""
    W = 1 << lw
    for B in _blocks(world):
        total, bounds = B * world, sw.plan_bounds(B, chunks)
        piece_of_offset = np.zeros(B, np.int64)
        for c, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
            piece_of_offset[lo:hi] = c
        for rank in range(world):
            arrival = np.tile(piece_of_offset, world)
            arrival[rank * B:(rank + 1) * B] = -1
            want = [int(arrival[p * W:(p + 1) * W].max()) for p in range(-(-total // W))]
            got = sw.panel_ready_piece(total, world, rank, lw, bounds)
            assert got == want, (B, rank)
            # every panel has exactly one stage, and the local ones are those wholly inside the own block
            assert len(got) == -(-total // W) and all(-1 <= c < len(bounds) - 1 for c in got)
            inside = [rank * B <= p * W and min((p + 1) * W, total) <= (rank + 1) * B for p in range(len(got))]
            assert [c == -1 for c in got] == inside


@pytest.mark.parametrize("rows,rpb", [(1006, 512), (1600, 512), (2011, 512), (4267, 512), (6400, 1024)])
def test_piece_row_blocks_hold_their_rows(rows, rpb):
    """after the row blocks of pieces 0 .. r every row of those pieces is final: the blocks of piece r end at or after its last row"""
    for chunks in (1, 2, 3, 4):
        b = sw.plan_bounds(rows, chunks)
        rb = sw.piece_row_blocks(rows, rpb, b)
        assert rb[0] == 0 and rb[-1] == -(-rows // rpb) and all(x <= y for x, y in zip(rb[:-1], rb[1:]))
        for r in range(len(b) - 1):
            assert min(rb[r + 1] * rpb, rows) >= b[r + 1]


@pytest.mark.parametrize("world", sw.WORLDS)
def test_numpy_world_reproduces_the_unsharded_model(world):
    """blocks padded as Partition pads them, K applied block by block: three fixed steps equal HandleModel.iterate of the whole LP"""
    lp = sw.world_lp()
    m = hm.HandleModel(lp)
    x, y = hm.start_point(lp, sw.START_SEED)
    m.set_iterate(x, y)
    m.set_step(m.eta0, 1.25, 1.0, 0)
    m.iterate(3, False)
    nw = sw.NumpyWorld(lp, world)
    assert (nw.part.Bn, nw.part.Bm) == _blocks(world) and nw.part.np_ > lp.n          # every world pads n
    assert (nw.part.mp > lp.m) == (world == 3)
    nw.set_iterate(x, y)
    nw.iterate(3, m.eta0, 1.25)
    gx, gy = nw.get_iterate()
    assert np.abs(gx - m.x).max() <= 1e-13 * (1 + np.abs(m.x).max())
    assert np.abs(gy - m.y).max() <= 1e-13 * (1 + np.abs(m.y).max())
    assert np.abs(m.x - x).max() > 1e-2                                                # (the iteration moved)


def test_adaptive_decisions_are_robust():
    """13 adaptive steps from the start the GPU tests use: every accept / reject decision is at least 5 % away from its threshold,
    500 times the float32 bound on eta (rtol 1e-4): no engine within its tolerance can decide otherwise"""
    mg = sw.decision_margins(sw.world_lp(), sw.START_SEED, sw.STEP["factor"], sw.STEP["omega"], sw.STEP["k0"], 13)
    assert min(m for _, m in mg) >= 0.05, mg


def test_retry_step_is_rejected():
    """50 times the safe step: the rule's eta_bar of such a step is eta * (1 + small) -- the step itself dominates both sums -- so the
    FIRST trial is accepted by a small margin, with eta' next to eta_bar, and the trial after it is rejected (late in a solve the rule
    shrinks eta by (k + 1)^-0.3 only).  Both margins are at least 1e-5: 10^5 float64 tolerances (1e-10 on eta)."""
    mg = sw.decision_margins(sw.world_lp(), sw.START_SEED, sw.RETRY_STEP["factor"], sw.RETRY_STEP["omega"], sw.RETRY_STEP["k0"], 2)
    assert [a for a, _ in mg] == [True, False], mg
    assert min(m for _, m in mg) >= 1e-5, mg


def test_directed_list_holds_every_case():
    """the cases the list was chosen for, from the contract alone (the GPU tests assert them again from what the library reports)"""
    props = {cfg[:4]: sw.config_properties(cfg[0], cfg[1], cfg[3]) for cfg in sw.CONFIGS}
    assert 24 <= len(sw.CONFIGS) <= 32 and len(props) == len(sw.CONFIGS)
    for prec in ("f32", "f64"):
        for key in ("empty_phase", "empty_piece", "unsplit_rank", "fully_split", "boundary_in_panel", "ragged_panel"):
            assert any(p[key] for c, p in props.items() if c[2] == prec), (prec, key)
        assert {c[0] for c in props if c[2] == prec} == set(sw.WORLDS) and {c[1] for c in props if c[2] == prec} == set(sw.LWS)
        assert {c[3] for c in props if c[2] == prec} == {1, 2, 3, 4}
    assert all(p["fully_split"] for c, p in props.items() if c[1] in (6, 8))
    assert all(p["empty_phase"] for c, p in props.items() if c[1] == 11 and c[3] > 1)
    p = sw.config_properties(8, 8, 4)
    assert p["stages"][0][7] == [4, 0, 7, 7, 14] and p["row_blocks"][1] == [0, 1, 1, 2, 2]
    assert sw.config_properties(8, 8, 3)["row_blocks"][1] == [0, 1, 2, 2]
    assert any(c[2] == "mixed" and c[0] == 4 for c in props)
    assert {c[0] for c in sw.CONFIGS if c[4]} == set(sw.WORLDS)                       # the option switches once per world
    lp = sw.world_lp()
    assert lp.m_ineq == 5120 and 3 * 1600 < lp.m_ineq < 4 * 1600
    assert np.isinf(lp.l).any() and np.isinf(lp.u).any() and (lp.l == lp.u).any()              # free, one-sided and fixed variables
