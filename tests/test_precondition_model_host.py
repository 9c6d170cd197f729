"""``tests/precondition_model.py`` is pinned to the reference before it judges the device kernels: at float32 it reproduces every
case of ``tests/golden/ruiz.npz`` to ``test_ruiz_vs_golden``'s tolerances.  (Not to the bit: the fixtures carry the float32 square
root of the CPU torch that wrote them, which is not IEEE's in every element -- the model, like the kernels, rounds correctly -- and
the difference, 1 ulp after one sweep, is 5 ulp at most after twenty.)  Its two copies are transposes of each other bit for bit, and
the inputs of the end-to-end sweep tests keep their distance from the early exit's threshold.  No GPU."""
import math

import numpy as np
import pytest

from tests import precondition_model as pm

TYPES = pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])


def close(a, b, rtol):
    """tests/test_gpu_parity.py's ``close``"""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=rtol * max(1.0, float(np.max(np.abs(b))) if b.size else 1.0))


def csr_of_dense(K):
    """``CsrPair.from_dense``: the entries that are not 0, row by row"""
    nz = K != 0
    rp = np.zeros(K.shape[0] + 1, np.int64)
    np.cumsum(nz.sum(1), out=rp[1:])
    return nz, rp, np.nonzero(nz)[1].astype(np.int32), K[nz]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_model_reproduces_the_reference_fixtures(golden):
    g = golden("ruiz.npz")
    cases = sorted({"/".join(k.split("/")[:3]) for k in g.z.files})
    assert len(cases) >= 8
    empty_rows = empty_cols = 0
    for case in cases:
        r = g.group(case)
        iters = int(case.rsplit("it", 1)[1])
        K = r["K"]
        assert K.dtype == np.float32
        nz, rp, ci, va = csr_of_dense(K)
        empty_rows += int((nz.sum(1) == 0).sum())
        empty_cols += int((nz.sum(0) == 0).sum())
        s = pm.equilibrate(rp, ci, va, K.shape[1], np.float32, max_iter=iters)
        assert s.sweeps == iters                                  # (no fixture ends early)
        close(s.d_col, r["D_col"], 1e-5)
        close(s.d_row, r["D_row"], 1e-5)
        Ks = np.zeros_like(K)
        Ks[nz] = s.val
        np.testing.assert_allclose(Ks, r["K_s"], rtol=1e-5, atol=1e-7)
        Kt = np.zeros_like(K.T)
        Kt[pm.row_of(s.t_rp), s.t_ci] = s.t_val
        assert same_bits(np.ascontiguousarray(Kt.T), Ks)
        for got, key in zip(s.scale(r["c"], r["q"], r["l"], r["u"]), ("c_s", "q_s", "l_s", "u_s")):
            assert got.dtype == np.float32
            np.testing.assert_allclose(got, r[key], rtol=1e-5)
    assert empty_rows >= 1 and empty_cols >= 1                    # the factor-1 rule is among what the fixtures pin


@TYPES
@pytest.mark.parametrize("pock_chambolle", [False, True], ids=["ruiz", "ruiz+pc"])
@pytest.mark.parametrize("name", sorted(pm.sweep_cases()))
def test_the_two_copies_are_transposes_bit_for_bit(name, pock_chambolle, T):
    m, n, rp, ci, va, max_iter = pm.sweep_cases()[name]
    s = pm.equilibrate(rp, ci, va, n, T, max_iter=max_iter, pock_chambolle=pock_chambolle)
    assert s.val.dtype == s.t_val.dtype == s.d_row.dtype == s.d_col.dtype == T
    assert same_bits(s.t_val, s.val[s.perm])
    # the permutation is the transpose: item p of K' is (column, row) of item perm[p] of K
    assert np.array_equal(pm.row_of(s.t_rp), ci[s.perm]) and np.array_equal(s.t_ci, pm.row_of(rp)[s.perm])
    assert np.isfinite(s.val).all() and (s.d_row > 0).all() and (s.d_col > 0).all()
    # Ks = diag(D_row) K diag(D_col) to the roundings of the sweeps (two divisions per sweep and two in the pass)
    want = va * s.d_row.astype(np.float64)[pm.row_of(rp)] * s.d_col.astype(np.float64)[ci]
    assert np.allclose(s.val.astype(np.float64), want, rtol=(4 * s.sweeps + 8) * np.finfo(T).eps, atol=0)


def kernel_order_sum(items):
    """k_row_l1_factors for one row, lane by lane in plain Python floats"""
    s = [0.0] * 8
    for k, v in enumerate(items):                                 # (k ascending: a lane's items in their order)
        s[k % 8] += abs(v)
    for off in (4, 2, 1):
        s = [s[lt] + s[lt ^ off] for lt in range(8)]
    assert len(set(s)) == 1                                       # every lane ends with the same bits
    return s[0]


def test_lane_order_sum_is_the_kernels_order():
    # by hand: lane 0 adds 2^53 + 1 -> 2^53 (a tie, to even), lanes 1..7 hold 1; distance 4: 2^53 + 1 -> 2^53 and three times 2;
    # distance 2: 2^53 + 2 and 4; distance 1: 2^53 + 6 -- the exact sum is 2^53 + 8
    one_row = np.array([2.0 ** 53] + [1.0] * 8)
    assert pm.lane_order_sums(np.array([0, 9]), one_row)[0] == 2.0 ** 53 + 6 == kernel_order_sum(one_row)
    rng = np.random.default_rng(8)
    lens = list(range(0, 41)) + [63, 64, 65, 300]
    rows = [10.0 ** rng.uniform(-8, 8, k) * rng.choice([-1.0, 1.0], k) for k in lens]
    rp = np.cumsum([0] + lens)
    got = pm.lane_order_sums(rp, np.concatenate(rows))
    assert [float(v) for v in got] == [kernel_order_sum(r) for r in rows]
    assert sum(float(g) != math.fsum(np.abs(r)) for g, r in zip(got, rows)) >= 10          # the order shows in these rows
    f = pm.row_l1_factors(rp, np.concatenate(rows).astype(np.float32), np.float32)
    assert f.dtype == np.float32 and f[0] == 1 and f[1] == np.float32(np.sqrt(np.float64(np.float32(abs(rows[1][0])))))


@TYPES
def test_threshold_rule_of_the_row_factors(T):
    """``r < T(eps)`` gives 1, ``r == T(eps)`` keeps r; stored zeros, a subnormal maximum and an empty row give 1"""
    rp, va, below, at, above = pm.threshold_rows(T)
    assert below < at == T(pm.EPS) < above and np.nextafter(at, T(0)) == below and np.nextafter(at, T(np.inf)) == above
    got = pm.row_scale_factors(rp, va, pm.EPS, T)
    assert got.dtype == T and list(got) == [T(1), at, above, T(1), T(1), T(1)]


@pytest.mark.parametrize("name", sorted(pm.sweep_cases()))
def test_sweep_inputs_stay_clear_of_the_exit_threshold(name):
    """The condition on the inputs of the end-to-end sweep tests: with the model in float64, no sweep ends with ``max |1 - r|``
    inside ``[eps / 2, 2 eps]`` -- so the sweep count cannot hang on the last bits of a factor, in either precision.  (Ruiz halves
    ``max |1 - r|`` per sweep once it converges, and a band that is 4 wide cannot be stepped over at that rate: the cases end either
    after sweep 1 with every row factor exactly 1, or at ``max_iter`` far above the band.)"""
    m, n, rp, ci, va, max_iter = pm.sweep_cases()[name]
    assert np.array_equal(va.astype(np.float32).astype(np.float64), va)        # both precisions start from the same matrix
    s64 = pm.equilibrate(rp, ci, va, n, np.float64, max_iter=max_iter)
    assert len(s64.devs) == s64.sweeps
    for k, d in enumerate(s64.devs):
        assert not (pm.EPS / 2 <= d <= 2 * pm.EPS), f"{name}: sweep {k + 1} ends with max|1-r| = {d!r}"
    s32 = pm.equilibrate(rp, ci, va, n, np.float32, max_iter=max_iter)
    assert s32.sweeps == s64.sweeps and s64.sweeps in (1, max_iter)


def test_sweep_cases_have_what_the_dense_fixtures_lack():
    cases = pm.sweep_cases()
    m, n, rp, ci, va, _ = cases["wide_300x200"]
    lens, hits = np.diff(rp), np.bincount(ci, minlength=n)
    assert (m, n) == (300, 200) and lens[11] == 0 and hits[7] == 0 and set(range(1, 41)) <= set(lens.tolist())
    assert np.abs(va[rp[23]:rp[24]]).max() < pm.EPS ** 2 and hits[31] > 10 and np.abs(va[ci == 31]).max() < pm.EPS ** 2
    live = np.abs(va)[np.abs(va) > pm.EPS ** 2]
    assert live.min() < 1e-5 and live.max() > 1e5 and (va < 0).any() and (va > 0).any()
    for i in range(m):
        assert (np.diff(ci[rp[i]:rp[i + 1]]) > 0).all()
    s = pm.equilibrate(rp, ci, va, n, np.float32)
    assert s.d_row[11] == 1 and s.d_col[7] == 1 and s.d_row[23] == 1 and s.d_col[31] == 1
    assert set(np.abs(cases["signs_96x64"][4]).tolist()) == {1.0}
    m, n, rp, ci, va, _ = cases["signs_96x64"]
    assert np.bincount(ci, minlength=n).min() > 0 and np.diff(rp).min() > 0 and pm.equilibrate(rp, ci, va, n, np.float64).sweeps == 1
