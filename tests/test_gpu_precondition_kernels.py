"""The preconditioner's device kernels on the MI355X, each called through the C ABI in float32 and float64 and compared with
``tests/precondition_model.py`` (plain numpy in the same precision, pinned to the reference's fixtures by
``tests/test_precondition_model_host.py``) on the same inputs: pdlp_csr_row_scale_factors, pdlp_csr_row_l1_factors, pdlp_csr_div_rows,
pdlp_csr_div_cols, pdlp_vec_muldiv, pdlp_vec_max_dev_from_one, pdlp_vec_sqdist; then ``equilibrate_matrix`` end to end,
``ops.primal_weight_update`` and pdlp_vec_project_lambda.

Factors, divisions and ``max |1 - r|`` are compared BIT FOR BIT: each result is one correctly rounded IEEE operation (a division, a
square root) or a max of T inputs, and the 1-norm is added in double in an order that depends on the row alone, which the model
repeats.  The sums of pdlp_vec_sqdist get a derived bound (``test_sqdist``).  Every output buffer starts as NaN, so an element that a
kernel skips shows.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import torchpdlp_amd as tp
from tests import precondition_model as pm
from tests.handle_model import project_lambda_box
from torchpdlp_amd import _native as N
from torchpdlp_amd.engine import _DT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
BITS = {np.dtype(np.float32): np.int32, np.dtype(np.float64): np.int64}
EPS = pm.EPS

# what one pass of a capped grid reaches, from the library's own constants: grid_for(n) launches min(ceil(n / BLOCK), MAX_GRID)
# workgroups of BLOCK threads; the row kernels give a row 8 lanes (grid_for(rows * 8))
_SRC = open(os.path.join(ROOT, "torchpdlp_amd", "csrc", "pdlp_hip.hip")).read()
BLOCK = int(re.search(r"constexpr int BLOCK = (\d+);", _SRC).group(1))
MAX_GRID = int(re.search(r"constexpr int MAX_GRID = (\d+);", _SRC).group(1))
assert re.search(r"inline int grid_for\(int64_t n\) \{ int64_t g = \(n \+ BLOCK - 1\) / BLOCK; .*g > MAX_GRID \? MAX_GRID : g", _SRC)
PASS_ITEMS = MAX_GRID * BLOCK                     # elements of one pass of an element-per-thread kernel
PASS_ROWS = PASS_ITEMS // pm.LANES                # rows of one pass of a row kernel: its stride
BIG_ROWS = PASS_ROWS + 37                         # a second pass of 37 rows: not a multiple of the stride
BIG_LEN = PASS_ITEMS + 77
assert BIG_ROWS % PASS_ROWS and BIG_LEN % PASS_ITEMS and BIG_ROWS < 1 << 17 and BIG_LEN < 1 << 20       # (stays a few ms of work)
LENGTHS = [1, 255, 256, 257, BIG_LEN]


def device():
    return torch.device("cuda", 0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device())


def host(t):
    return t.cpu().numpy()


def nan_like(n, T):
    return torch.full((int(n),), float("nan"), dtype=TORCH[T], device=device())


def call(name, *args):
    st = torch.cuda.current_stream(device())
    N.check(getattr(N.load(), name)(*args, st.cuda_stream), name)
    st.synchronize()


def ulps_apart(got, want):
    """distance in units of the last place of every pair of finite numbers of one sign (their bit patterns are ordered like them)"""
    I = BITS[got.dtype]
    ok = np.isfinite(got) & np.isfinite(want) & (np.signbit(got) == np.signbit(want))
    return np.abs(got.view(I)[ok].astype(np.int64) - want.view(I)[ok].astype(np.int64))


def assert_same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    I = BITS[got.dtype]
    bad = np.nonzero(got.view(I) != want.view(I))[0]
    print(f"{what} [{got.dtype.name}]: {bad.size} of {got.size} differ from the model; largest distance "
          f"{int(ulps_apart(got, want).max(initial=0))} ulp")
    assert bad.size == 0, f"{what}: first at {bad[:5]}: got {got[bad[:5]]!r}, model {want[bad[:5]]!r}"


# ---------------------------------------------------------------------------------------------------------------------------------
# the entry points on numpy arrays
# ---------------------------------------------------------------------------------------------------------------------------------
def gpu_row_scale_factors(T, rp, va, eps=EPS):
    rows = len(rp) - 1
    d_rp, d_va, out = dev(np.asarray(rp, np.int64)), dev(np.asarray(va, T)), nan_like(rows, T)
    call("pdlp_csr_row_scale_factors", _DT[TORCH[T]], rows, d_rp.data_ptr(), d_va.data_ptr(), float(eps), out.data_ptr())
    return host(out)


def gpu_row_l1_factors(T, rp, va):
    rows = len(rp) - 1
    d_rp, d_va, out = dev(np.asarray(rp, np.int64)), dev(np.asarray(va, T)), nan_like(rows, T)
    call("pdlp_csr_row_l1_factors", _DT[TORCH[T]], rows, d_rp.data_ptr(), d_va.data_ptr(), out.data_ptr())
    return host(out)


def gpu_div_rows(T, rp, va, norm):
    rows = len(rp) - 1
    d_rp, d_va, d_norm = dev(np.asarray(rp, np.int64)), dev(np.asarray(va, T)), dev(np.asarray(norm, T))
    call("pdlp_csr_div_rows", _DT[TORCH[T]], rows, d_rp.data_ptr(), d_va.data_ptr(), d_norm.data_ptr())
    return host(d_va)


def gpu_div_cols(T, ci, va, norm_full):
    d_ci, d_va, d_norm = dev(np.asarray(ci, np.int32)), dev(np.asarray(va, T)), dev(np.asarray(norm_full, T))
    call("pdlp_csr_div_cols", _DT[TORCH[T]], len(ci), d_ci.data_ptr(), d_va.data_ptr(), d_norm.data_ptr())
    return host(d_va)


def gpu_muldiv(T, a, b, op):
    d_a, d_b = dev(np.asarray(a, T)), dev(np.asarray(b, T))
    call("pdlp_vec_muldiv", _DT[TORCH[T]], len(a), d_a.data_ptr(), d_b.data_ptr(), op)
    return host(d_a)


def gpu_max_dev(T, v, work=None):
    work = torch.full((1,), float("nan"), dtype=torch.float64, device=device()) if work is None else work
    d_v, out = dev(np.asarray(v, T)), C.c_double(float("nan"))
    call("pdlp_vec_max_dev_from_one", _DT[TORCH[T]], len(v), d_v.data_ptr(), work.data_ptr(), C.byref(out))
    return out.value


def gpu_sqdist(T, a, b):
    work = torch.full((1040,), float("nan"), dtype=torch.float64, device=device())       # (ops.primal_weight_update's size)
    d_a, d_b, out = dev(np.asarray(a, T)), dev(np.asarray(b, T)), C.c_double(float("nan"))
    call("pdlp_vec_sqdist", _DT[TORCH[T]], len(a), d_a.data_ptr(), d_b.data_ptr(), work.data_ptr(), C.byref(out))
    return out.value


def check_row_kernels(T, rp, va, what):
    """the three row kernels on one matrix: the max-norm factors, the rows divided by them, the 1-norm factors"""
    va = np.asarray(va, T)
    want = pm.row_scale_factors(rp, va, EPS, T)
    got = gpu_row_scale_factors(T, rp, va)
    assert_same_bits(got, want, f"{what}: row_scale_factors")
    assert_same_bits(gpu_div_rows(T, rp, va, want), pm.div_rows(rp, va, want), f"{what}: div_rows")
    assert_same_bits(gpu_row_l1_factors(T, rp, va), pm.row_l1_factors(rp, va, T), f"{what}: row_l1_factors")
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the 8-lanes-per-row layout: row lengths, and where in the row the maximum sits
# ---------------------------------------------------------------------------------------------------------------------------------
ROW_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1000]


def rows_with_the_maximum_in_every_lane():
    """For every length L one row per place of the maximum: the first item, the last item, and for every lane lt < min(L, 8) the LAST
    item that lane reads (lt + 8 j).  The maximum is negative in every other row and differs from row to row"""
    rng = np.random.default_rng(14)
    rows, places = [], []
    for L in ROW_LENGTHS:
        at = sorted({0, L - 1} | {lt + 8 * ((L - 1 - lt) // 8) for lt in range(min(L, 8))}) if L else [None]
        for p in at:
            v = rng.uniform(0.2, 2.0, L) * rng.choice([-1.0, 1.0], L)
            if p is not None:
                v[p] = (3.0 + 0.37 * len(rows)) * (-1.0 if len(rows) % 2 else 1.0)
            rows.append(v)
            places.append((L, p))
    rp = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    return rp, np.concatenate(rows), places


@TYPES
def test_row_kernels_over_row_lengths_and_places_of_the_maximum(T):
    rp, va, places = rows_with_the_maximum_in_every_lane()
    lanes = {p % 8 for L, p in places if p is not None and L >= 9}
    assert lanes == set(range(8)) and {L for L, _ in places} == set(ROW_LENGTHS)
    assert any(p == 0 for L, p in places if L > 1) and any(p == L - 1 for L, p in places if L > 1)
    va = va.astype(T)
    mx = np.array([np.abs(va[a:b]).max(initial=0) for a, b in zip(rp[:-1], rp[1:])])
    neg = sum(va[a:b][np.abs(va[a:b]).argmax()] < 0 for a, b in zip(rp[:-1], rp[1:]) if b > a)
    assert abs(2 * neg - (len(rp) - 2)) <= 1                       # negative in half the rows
    got = check_row_kernels(T, rp, va, "row lengths")
    assert got[0] == 1 and len(set(got.tolist())) == len(got)      # the empty row; no two rows share a factor
    assert_same_bits(got[1:], np.sqrt(mx[1:].astype(np.float64)).astype(T), "factors from the rows' maxima")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. row counts: the lane-group, wave and workgroup edges, and a second pass of the capped grid
# ---------------------------------------------------------------------------------------------------------------------------------
@TYPES
@pytest.mark.parametrize("rows", [1, 7, 8, 9, 31, 32, 33, 255, 256, 257, BIG_ROWS])
def test_row_kernels_over_row_counts(rows, T):
    """0 to 11 items per row (1 or 2 in the case that needs a second pass of the grid: its last 37 rows)"""
    rng = np.random.default_rng(rows)
    lens = 1 + np.arange(rows) % 2 if rows == BIG_ROWS else (np.arange(rows) * 5 + 1) % 12
    rp = np.zeros(rows + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    va = (10.0 ** rng.uniform(-3, 3, int(rp[-1])) * rng.choice([-1.0, 1.0], int(rp[-1]))).astype(T)
    got = check_row_kernels(T, rp, va, f"{rows} rows")
    assert np.isfinite(got).all() and (rows < 12 or (got[lens == 0] == 1).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the threshold of the row factors
# ---------------------------------------------------------------------------------------------------------------------------------
@TYPES
def test_row_factors_at_the_threshold(T):
    rp, va, below, at, above = pm.threshold_rows(T)
    got = gpu_row_scale_factors(T, rp, va)
    assert_same_bits(got, pm.row_scale_factors(rp, va, EPS, T), "threshold rows")
    # sqrt(max) one below eps: 1; == eps: kept; one above: kept; stored zeros, a subnormal maximum, an empty row: 1
    assert list(got) == [T(1), at, above, T(1), T(1), T(1)]
    assert_same_bits(gpu_div_rows(T, rp, va, got), pm.div_rows(rp, va, got), "threshold rows divided")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. pdlp_csr_div_cols: the gather of the column factors
# ---------------------------------------------------------------------------------------------------------------------------------
def column_pattern(nnz, n=53, empty=3):
    """rows of 4 items in DESCENDING column order: column n - 1, which is in every row, then three of the others, dealt from
    shuffled decks of them so that every column comes round; column ``empty`` is in no row.  The last row is cut at ``nnz``"""
    rng = np.random.default_rng(nnz)
    others = np.setdiff1d(np.arange(n - 1), [empty])
    assert others.size % 3 == 0                                    # (a row never takes from two decks: no column twice in a row)
    decks = np.concatenate([rng.permutation(others) for _ in range(nnz // (4 * others.size // 3) + 1)]).reshape(-1, 3)
    rows = np.concatenate([np.full((len(decks), 1), n - 1), -np.sort(-decks, axis=1)], axis=1)
    return rows.reshape(-1)[:nnz].astype(np.int32)


@TYPES
@pytest.mark.parametrize("nnz", LENGTHS)
def test_div_cols(nnz, T):
    n, empty = 53, 3
    ci = column_pattern(nnz, n, empty)
    assert ci[0] == n - 1 and empty not in ci and (nnz < 255 or (np.bincount(ci, minlength=n)[np.arange(n) != empty] > 0).all())
    assert nnz < 4 or ci[0] > ci[1] > ci[2] > ci[3]
    rng = np.random.default_rng(nnz + 1)
    va = (10.0 ** rng.uniform(-3, 3, nnz) * rng.choice([-1.0, 1.0], nnz)).astype(T)
    norm = (1.1 + 0.37 * np.arange(n)).astype(T)                   # distinct, no power of two: a wrong gather cannot cancel
    norm[empty] = np.nan                                           # never gathered
    got = gpu_div_cols(T, ci, va, norm)
    assert np.isfinite(got).all()
    assert_same_bits(got, pm.div_cols(ci, va, norm), f"div_cols, {nnz} items")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. pdlp_vec_muldiv
# ---------------------------------------------------------------------------------------------------------------------------------
@TYPES
@pytest.mark.parametrize("op", [0, 1], ids=["mul", "div"])
@pytest.mark.parametrize("n", LENGTHS)
def test_vec_muldiv(n, op, T):
    """infinite bounds divided by a factor (``l / D_col``, ``u / D_col``), both zeros and a subnormal among ordinary numbers"""
    rng = np.random.default_rng(n + op)
    a = (10.0 ** rng.uniform(-3, 3, n) * rng.choice([-1.0, 1.0], n)).astype(T)
    special = [np.inf, -np.inf, -0.0, 0.0, np.finfo(T).smallest_subnormal * 5]
    for k, s in enumerate(special):
        a[(k * 97 + n - 1) % n] = s                                # spread over the vector; the last element is one of them
    b = (0.3 + 0.37 * (np.arange(n) % 1000) + rng.uniform(0, 0.1, n)).astype(T)
    got, want = gpu_muldiv(T, a, b, op), pm.muldiv(a, b, op)
    assert_same_bits(got, want, f"muldiv op {op}, {n} elements")
    assert not np.isnan(got).any() and (n < 255 or (np.isinf(got).sum() == 2 and np.signbit(got[got == 0]).sum() == 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. pdlp_vec_max_dev_from_one
# ---------------------------------------------------------------------------------------------------------------------------------
@TYPES
@pytest.mark.parametrize("n", [0] + LENGTHS)
def test_max_dev_from_one(n, T):
    """the maximum at the first index, at the last one and inside the tail of the grid-stride loop; values all below 1, all above 1
    (|1 - v| rounds in T for the planted ones: 0.1, 3.3) and all exactly 1"""
    if n == 0:
        assert gpu_max_dev(T, np.zeros(0, T)) == 0.0               # no launch: the memset alone
        return
    rng = np.random.default_rng(n)
    tail = PASS_ITEMS + 5 if n > PASS_ITEMS else max(n - 2, 0)
    for lo, hi, planted in ((0.5, 0.99, 0.1), (1.01, 1.5, 3.3)):
        for at in sorted({0, n - 1, tail}):
            v = rng.uniform(lo, hi, n).astype(T)
            v[at] = planted
            got, want = gpu_max_dev(T, v), pm.max_dev_from_one(v)
            assert want == float(abs(T(1) - T(planted))) and want > 0.5
            assert got == want, f"{n} elements, maximum at {at}: got {got!r}, model {want!r}"
    assert gpu_max_dev(T, np.ones(n, T)) == 0.0


@TYPES
def test_max_dev_from_one_twice_on_one_work_buffer(T):
    work = torch.full((1,), float("nan"), dtype=torch.float64, device=device())
    n = 1000
    v1 = np.linspace(0.6, 1.4, n).astype(T)
    v1[n - 1] = 0.1
    v2 = np.linspace(0.8, 1.2, n).astype(T)
    first, second = gpu_max_dev(T, v1, work), gpu_max_dev(T, v2, work)
    assert first == pm.max_dev_from_one(v1) and second == pm.max_dev_from_one(v2) and 0 < second < first
    assert gpu_max_dev(T, np.zeros(0, T), work) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. pdlp_vec_sqdist
# ---------------------------------------------------------------------------------------------------------------------------------
SQDIST_RATIOS = {}


@TYPES
@pytest.mark.parametrize("n", [1, 255, 256, 257, 256 * 256 + 1])
def test_sqdist(n, T):
    """Against the float64 sum of ``(double)(T)(a - b)`` squared, added exactly (``math.fsum``) and rounded once.

    The bound.  The kernel's terms are the reference's: the difference rounded to T, widened, multiplied by itself in double -- one
    correctly rounded operation on either side (exact for float32).  The kernel adds them in double in two levels (a thread its
    strided elements, the workgroup's 256 sums in a tree, then the at most 256 workgroup sums by one workgroup in a tree), the
    padding of the trees being zeros, which add nothing.  A sum of n non-negative terms by n - 1 rounded additions IN ANY ORDER is
    within gamma(n - 1) S of their exact sum S, gamma(k) = k u / (1 - k u), u = 2^-53; the reference is within u S of it.  So
    ``|got - ref| <= (gamma(n - 1) + u) S <= n u S / (1 - n u)``, whatever the two-level order: its constant is 1."""
    rng = np.random.default_rng(n)
    a = (10.0 ** rng.uniform(-6, 6, n) * rng.choice([-1.0, 1.0], n)).astype(T)
    b = (10.0 ** rng.uniform(-6, 6, n) * rng.choice([-1.0, 1.0], n)).astype(T)
    terms = pm.sqdist_terms(a, b)
    ref = math.fsum(terms.tolist())
    u = 2.0 ** -53
    bound = n * u * ref / (1 - n * u)
    got = gpu_sqdist(T, a, b)
    ratio = abs(got - ref) / bound
    SQDIST_RATIOS[(np.dtype(T).name, n)] = ratio
    print(f"sqdist [{np.dtype(T).name}] n = {n}: got {got!r}, reference {ref!r}, |error| / bound = {ratio:.3g}; "
          f"largest so far {max(SQDIST_RATIOS.values()):.3g}")
    assert ref > 0 and abs(got - ref) <= bound
    if n == 1:
        assert got == ref
    # the same vector twice: exactly 0
    assert gpu_sqdist(T, a, a) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the sweeps end to end
# ---------------------------------------------------------------------------------------------------------------------------------
@TYPES
@pytest.mark.parametrize("pock_chambolle", [False, True], ids=["ruiz", "ruiz+pc"])
@pytest.mark.parametrize("name", sorted(pm.sweep_cases()))
def test_equilibrate_matrix_against_the_model(name, pock_chambolle, T):
    """``D_row``, ``D_col``, both value arrays and the sweep count of ``equilibrate_matrix`` are the model's, bit for bit: every
    kernel of the sweeps is (tests above), and the loop only chains them.  The inputs keep the sweep count away from its threshold
    (tests/test_precondition_model_host.py::test_sweep_inputs_stay_clear_of_the_exit_threshold)"""
    m, n, rp, ci, va, max_iter = pm.sweep_cases()[name]
    K = tp.CsrPair(m, n, torch.from_numpy(rp), torch.from_numpy(ci), torch.from_numpy(va.astype(T))).to(device())
    before = host(K.val).copy()
    Ks, scaling = tp.equilibrate_matrix(K, device(), max_iter=max_iter, eps=EPS, pock_chambolle=pock_chambolle)
    want = pm.equilibrate(rp, ci, va, n, T, max_iter=max_iter, eps=EPS, pock_chambolle=pock_chambolle)
    print(f"{name} [{np.dtype(T).name}]: {scaling.sweeps} sweeps, model {want.sweeps}; last max|1-r| {want.devs[-1]:.3g}")
    assert scaling.sweeps == want.sweeps and want.sweeps in (1, max_iter)
    assert np.array_equal(host(Ks.rowptr), want.rp) and np.array_equal(host(Ks.colidx), want.ci)
    assert np.array_equal(host(Ks.t_rowptr), want.t_rp) and np.array_equal(host(Ks.t_colidx), want.t_ci)
    assert_same_bits(host(scaling.d_row), want.d_row, "D_row")
    assert_same_bits(host(scaling.d_col), want.d_col, "D_col")
    assert_same_bits(host(Ks.val), want.val, "K")
    assert_same_bits(host(Ks.t_val), want.t_val, "K'")
    # the K' copy holds the bits of the K copy under the transpose permutation (the library's own, and the model's)
    assert_same_bits(host(Ks.t_val), host(Ks.val)[host(K.transpose_perm())], "K' against K[perm]")
    assert np.array_equal(host(K.transpose_perm()), want.perm)
    assert np.array_equal(host(K.val), before)                     # the caller's matrix is untouched


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. ops.primal_weight_update (pdlp_vec_sqdist twice, then the host formula)
# ---------------------------------------------------------------------------------------------------------------------------------
def primal_weight_64(x_prev, x, y_prev, y, omega, theta):
    """enhancements.py:73-78 in float64 from exactly added distances; ``(omega_new, |log(dy / dx)|, |log omega|)``"""
    dx = math.sqrt(math.fsum(((x_prev.astype(np.float64) - x) ** 2).tolist()))
    dy = math.sqrt(math.fsum(((y_prev.astype(np.float64) - y) ** 2).tolist()))
    if not (dx > 0 and dy > 0):
        return omega, 0.0, 0.0
    lr, lw = math.log(dy / dx), math.log(omega)
    return math.exp(theta * lr + (1 - theta) * lw), abs(lr), abs(lw)


@TYPES
@pytest.mark.parametrize("nx,ny", [(256 * 256 - 3, 256 * 256 + 3), (300, 70001), (1, 257)], ids=["cap", "small+over", "one"])
def test_primal_weight_update(nx, ny, T):
    """Lengths on both sides of pdlp_vec_sqdist's cap of 256 workgroups (256 * 256 elements fill them once).

    The bound, with u the unit roundoff of T and theta = 1/2.  The library rounds to T: the differences (u relative in each of them,
    so in each norm), the two norms and their ratio -- 5 u relative, so 5 u absolute in ``lr = log(dy / dx)`` -- and lr itself
    (u |lr|); omega (u absolute in ``lw = log omega``) and lw (u |lw|); the two products (u theta |lr|, u (1 - theta) |lw|), their
    sum e (u |e|) and the result (u relative).  An absolute error of the exponent is a relative one of the result.  The distances
    come from sums within ``n 2^-53`` relative (test_sqdist), half of that in a norm; libm's log and exp, on either side, are
    within 2^-52 relative.  First order, times 1.01 for the rest."""
    theta, omega = 0.5, float(T(1.7))
    rng = np.random.default_rng(nx + ny)
    vec = lambda n, s: (rng.standard_normal(n) * s).astype(T)
    x_prev, x, y_prev, y = vec(nx, 3.0), vec(nx, 3.0), vec(ny, 0.02), vec(ny, 0.02)
    d = lambda v: dev(v)
    got = float(tp.primal_weight_update(d(x_prev), d(x), d(y_prev), d(y), omega, theta))
    want, lr, lw = primal_weight_64(x_prev, x, y_prev, y, omega, theta)
    u = float(np.finfo(T).eps) / 2
    e = abs(math.log(want))
    allow = 1.01 * (u * (5 * theta + 2 * theta * lr + (1 - theta) * (1 + 2 * lw) + e + 1) + theta * (nx + ny) * 2.0 ** -54
                    + 2.0 ** -52 * 2 * (theta * lr + (1 - theta) * lw + 1))
    print(f"omega [{np.dtype(T).name}] {nx}, {ny}: got {got!r}, float64 {want!r}, relative error / bound = {abs(got - want) / want / allow:.3g}")
    assert lr > 1 and abs(got - want) <= allow * want
    # no movement of x, or of y: the guard keeps the old omega
    assert float(tp.primal_weight_update(d(x), d(x), d(y_prev), d(y), omega, theta)) == omega
    assert float(tp.primal_weight_update(d(x_prev), d(x), d(y), d(y), omega, theta)) == omega


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. pdlp_vec_project_lambda in both precisions (tests/test_gpu_parity.py has it in float32, through ops.project_lambda_box on a
# golden LP): the four bound classes side by side across workgroup edges, g of both signs and zero, against helpers.py's rule as
# tests/handle_model.py restates it
# ---------------------------------------------------------------------------------------------------------------------------------
@TYPES
@pytest.mark.parametrize("n", [1, 600, BIG_LEN])
def test_vec_project_lambda(n, T):
    i = np.arange(n)
    rng = np.random.default_rng(n)
    l = np.where(i % 4 >= 2, -np.inf, rng.uniform(-2, 0, n)).astype(T)           # boxed, lower only, upper only, free, boxed, ...
    u = np.where(i % 2 == 1, np.inf, rng.uniform(0, 2, n)).astype(T)
    g = (rng.uniform(0.1, 5, n) * np.array([-1.0, 0.0, 1.0])[(i // 4) % 3]).astype(T)
    if n >= 600:
        assert all(((np.isneginf(l) == a) & (np.isposinf(u) == b) & (np.sign(g) == sg)).any() for a in (0, 1) for b in (0, 1) for sg in (-1, 0, 1))
    d_g, d_l, d_u, out = dev(g), dev(l), dev(u), nan_like(n, T)
    call("pdlp_vec_project_lambda", _DT[TORCH[T]], n, d_g.data_ptr(), d_l.data_ptr(), d_u.data_ptr(), out.data_ptr())
    got = host(out)
    assert got.dtype == T and np.array_equal(got, project_lambda_box(g, l, u))
