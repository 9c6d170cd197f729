"""A plain numpy model of the preconditioner's device kernels (``pdlp_kernels_small.inc``: k_row_scale_factors, k_row_l1_factors,
k_div_rows, k_div_cols, k_muldiv, k_max_dev_from_one) and of the sweep loop that ``torchpdlp_amd.precondition`` builds from them,
over CSR triples, in the working precision ``T`` (``np.float32`` or ``np.float64``).

Every operation is a max, one division or one square root of a ``T`` value -- IEEE operations that numpy rounds correctly, so none
depends on an order -- apart from the 1-norm, which is added in double in the kernel's own order (``lane_order_sums``).  The judge of
``tests/test_gpu_precondition_kernels.py``; ``tests/test_precondition_model_host.py`` pins it to the reference's fixtures first.
"""
from dataclasses import dataclass, field

import numpy as np

LANES = 8            # lanes per row of the row kernels: lane lt takes items rp[i] + lt, + 8, ...


def row_of(rp):
    """the row of every item"""
    rp = np.asarray(rp, np.int64)
    return np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))


def csr_transpose(rp, ci, n):
    """``(t_rp, t_ci, perm)``: CSR pattern of the transpose, the rows of a column in their original order; ``t_val = val[perm]``"""
    ci = np.asarray(ci, np.int64)
    perm = np.argsort(ci, kind="stable")
    t_rp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(ci, minlength=n), out=t_rp[1:])
    return t_rp, row_of(rp)[perm].astype(np.int32), perm


def row_abs_max(rp, va):
    """max |.| of every row in the type of ``va``; 0 for an empty row"""
    mx = np.zeros(len(rp) - 1, va.dtype)
    np.maximum.at(mx, row_of(rp), np.abs(va))
    return mx


def row_scale_factors(rp, va, eps, T):
    """enhancements.py:49-50: ``r = sqrt(max |.|)`` (the square root taken in double and rounded to T: the same value as T's own
    correctly rounded square root), 1 where ``r < T(eps)`` -- ``r == T(eps)`` keeps r"""
    va = np.asarray(va, T)
    r = np.sqrt(row_abs_max(rp, va).astype(np.float64)).astype(T)
    return np.where(r < T(eps), T(1), r)


def lane_order_sums(rp, va):
    """sum |.| of every row in double, in k_row_l1_factors' order: lane lt adds its items ``rp[i] + lt, + 8, ...`` in that order from
    0, the eight sums meet in a butterfly over lane distances 4, 2, 1 (``a + b == b + a``: every lane ends with the same bits)"""
    rp = np.asarray(rp, np.int64)
    rows, length = rp.size - 1, np.diff(rp)
    a = np.abs(np.asarray(va).astype(np.float64))
    s = np.zeros((rows, LANES))
    for k in range(int(length.max(initial=0))):                   # item k of its row: lane k % 8, its (k // 8)-th addition
        live = np.nonzero(length > k)[0]
        s[live, k % LANES] += a[rp[live] + k]
    lane = np.arange(LANES)
    for off in (4, 2, 1):
        s = s + s[:, lane ^ off]
    return s[:, 0]


def row_l1_factors(rp, va, T):
    """the Pock-Chambolle factors: ``T(sqrt(sum |.|))``, 1 where the sum is 0"""
    s = lane_order_sums(rp, np.asarray(va, T))
    return np.where(s > 0.0, np.sqrt(np.where(s > 0.0, s, 1.0)).astype(T), T(1))


def div_rows(rp, va, norm):
    return va / norm[row_of(rp)]


def div_cols(ci, va, norm_full):
    return va / norm_full[np.asarray(ci, np.int64)]


def muldiv(a, b, op):
    """pdlp_vec_muldiv: ``a * b`` (op 0) or ``a / b`` (op 1)"""
    with np.errstate(all="ignore"):
        return a / b if op else a * b


def max_dev_from_one(v):
    """``max |1 - v|`` with the difference taken in the type of ``v``, widened to double; 0 for no elements"""
    return float(np.max(np.abs(v.dtype.type(1) - v), initial=0.0))


def sqdist_terms(a, b):
    """the terms of pdlp_vec_sqdist: ``a - b`` rounded to the vectors' type, squared in double"""
    with np.errstate(all="ignore"):
        d = (a - b).astype(np.float64)
    return d * d


def threshold_maximum(r, T):
    """a T number whose square root, rounded to T, is ``r``"""
    r = T(r)
    for mx in (T(r * r), np.nextafter(T(r * r), T(0)), np.nextafter(T(r * r), T(np.inf))):
        if np.sqrt(np.float64(mx)).astype(T) == r:
            return mx
    raise AssertionError("no T number has this square root")


def threshold_rows(T, eps=1e-6):
    """``(rp, va, below, at, above)``: six rows whose ``sqrt(max |.|)`` in T is the T number just below ``T(eps)``, ``T(eps)`` itself
    (its maximum negative, and not the row's only item) and the one just above; then a row of stored zeros, a row with a subnormal
    maximum and an empty row"""
    at = T(eps)
    below, above = np.nextafter(at, T(0)), np.nextafter(at, T(np.inf))
    mx = [threshold_maximum(w, T) for w in (below, at, above)]
    tiny = np.finfo(T).smallest_subnormal
    rows = [[mx[0]], [mx[1] / 2, -mx[1]], [mx[2]], [0.0, -0.0], [tiny * 3, -tiny], []]
    rp = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    return rp, np.array([v for r in rows for v in r], T), below, at, above


@dataclass
class Scaled:
    """what ``equilibrate`` returns: the two scaled CSR copies (patterns shared with the input), the factors with
    ``Ks = diag(d_row) K diag(d_col)``, the Ruiz sweeps run and the ``max |1 - r|`` each of them ended with"""
    rp: np.ndarray
    ci: np.ndarray
    val: np.ndarray
    t_rp: np.ndarray
    t_ci: np.ndarray
    t_val: np.ndarray
    perm: np.ndarray
    d_row: np.ndarray
    d_col: np.ndarray
    sweeps: int
    devs: list = field(default_factory=list)

    def scale(self, c, q, l, u):
        """``c * D_col, q * D_row, l / D_col, u / D_col`` (enhancements.py:64-67)"""
        return muldiv(c, self.d_col, 0), muldiv(q, self.d_row, 0), muldiv(l, self.d_col, 1), muldiv(u, self.d_col, 1)


def equilibrate(rp, ci, va, n, T, max_iter=20, eps=1e-6, pock_chambolle=False):
    """``torchpdlp_amd.precondition.equilibrate`` call by call: per sweep the row factors of K, ``D_row /= r``, K's rows and K''s
    columns divided by them, the same from K' for the columns, then the early exit on ``max |1 - r|`` of the ROW factors alone (quirk
    Q3; the comparison with ``eps`` is the host's, in double); with ``pock_chambolle`` one pass by the 1-norm factors, both taken
    before either division, composed into the same factors"""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int32)
    va = np.array(va, dtype=T)
    m = rp.size - 1
    t_rp, t_ci, perm = csr_transpose(rp, ci, n)
    t_va = va[perm]
    d_row, d_col = np.ones(m, T), np.ones(n, T)
    sweeps, devs = 0, []
    for _ in range(int(max_iter)):
        sweeps += 1
        r = row_scale_factors(rp, va, eps, T)
        d_row = muldiv(d_row, r, 1)
        va = div_rows(rp, va, r)
        t_va = div_cols(t_ci, t_va, r)
        c = row_scale_factors(t_rp, t_va, eps, T)
        d_col = muldiv(d_col, c, 1)
        t_va = div_rows(t_rp, t_va, c)
        va = div_cols(ci, va, c)
        devs.append(max_dev_from_one(r))
        if devs[-1] < eps:
            break
    if pock_chambolle:
        r, c = row_l1_factors(rp, va, T), row_l1_factors(t_rp, t_va, T)
        d_row = muldiv(d_row, r, 1)
        va = div_rows(rp, va, r)
        t_va = div_cols(t_ci, t_va, r)
        d_col = muldiv(d_col, c, 1)
        t_va = div_rows(t_rp, t_va, c)
        va = div_cols(ci, va, c)
    return Scaled(rp, ci, va, t_rp, t_ci, t_va, perm, d_row, d_col, sweeps, devs)


# ---------------------------------------------------------------------------------------------------------------------------------
# the sparse matrices of the end-to-end sweep tests: float64 values that are float32 numbers, so both precisions start from the same
# matrix.  The sweep count is a decision at a threshold: every case is chosen so that, with the model in float64, no sweep ends
# with max |1 - r| inside [eps / 2, 2 eps] (tests/test_precondition_model_host.py asserts it, away from the card)
# ---------------------------------------------------------------------------------------------------------------------------------
EPS = 1e-6


def _f32(v):
    return np.asarray(v, np.float32).astype(np.float64)


def _sparse_300x200(seed, lo, hi):
    """300 x 200, rows of 1 to 40 items with magnitudes 10^U(lo, hi) of both signs; row 11 and column 7 are empty, row 23 and column
    31 hold only entries far below eps^2 (their factors stay 1, whatever the sweeps do to them)"""
    m, n = 300, 200
    rng = np.random.default_rng(seed)
    lens = 1 + (np.arange(m) * 7) % 40
    lens[11] = 0
    live = np.setdiff1d(np.arange(n), [7, 31])
    rp = np.zeros(m + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(live, k, replace=False)) for k in lens]).astype(np.int32)
    va = 10.0 ** rng.uniform(lo, hi, ci.size) * rng.choice([-1.0, 1.0], ci.size)
    va[rp[23]:rp[24]] = 10.0 ** rng.uniform(-24, -20, lens[23]) * rng.choice([-1.0, 1.0], lens[23])
    # column 31: one tiny entry at the end of every seventh row (the rows stay sorted: 31 is put where it belongs)
    rows = [i for i in range(0, m, 7) if lens[i] > 0 and i != 23]
    out_ci, out_va, out_len = [], [], lens.copy()
    for i in range(m):
        c_i, v_i = ci[rp[i]:rp[i + 1]], va[rp[i]:rp[i + 1]]
        if i in rows:
            at = int(np.searchsorted(c_i, 31))
            c_i = np.insert(c_i, at, 31)
            v_i = np.insert(v_i, at, 10.0 ** rng.uniform(-24, -20) * rng.choice([-1.0, 1.0]))
            out_len[i] += 1
        out_ci.append(c_i)
        out_va.append(v_i)
    rp = np.zeros(m + 1, np.int64)
    np.cumsum(out_len, out=rp[1:])
    return m, n, rp, np.concatenate(out_ci).astype(np.int32), _f32(np.concatenate(out_va))


def _signs(m, n, per_row, seed):
    """+-1 in ``per_row`` places of every row, every column hit: already equilibrated, the first sweep's factors are all 1"""
    rng = np.random.default_rng(seed)
    cols = [np.sort(np.unique(np.concatenate([[i % n], rng.choice(n, per_row - 1, replace=False)]))) for i in range(m)]
    rp = np.zeros(m + 1, np.int64)
    np.cumsum([len(c) for c in cols], out=rp[1:])
    ci = np.concatenate(cols).astype(np.int32)
    assert m >= n and np.bincount(ci, minlength=n).min() > 0
    return m, n, rp, ci, rng.choice([-1.0, 1.0], ci.size)


def _one_by_one(v):
    return 1, 1, np.array([0, 1], np.int64), np.array([0], np.int32), _f32([v])


def sweep_cases():
    """name -> ``(m, n, rp, ci, va64, max_iter)``.  A 1 x 1 matrix v takes v to v^(1/4) per sweep, so its ``max |1 - r|`` falls by
    exactly 4 per sweep and cannot step over the band [eps / 2, 2 eps], which is 4 wide: the 1 x 1 cases end at ``max_iter`` sweeps
    far above the band, or hold a value below eps^2 and end after sweep 1 with the factor 1"""
    return {
        "wide_300x200": (*_sparse_300x200(3, -6, 6), 20),
        "mild_300x200": (*_sparse_300x200(4, -0.5, 0.5), 12),
        "signs_96x64": (*_signs(96, 64, 5, 5), 20),
        "one_by_one": (*_one_by_one(-3.7), 5),
        "one_by_one_tiny": (*_one_by_one(3e-15), 20),
    }
