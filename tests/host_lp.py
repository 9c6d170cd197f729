"""LPs held on the host for tests that drive a PdlpEngine call by call (tests/test_gpu_halpern.py, tests/test_gpu_sequences.py) and
for the float64 model of the handle (tests/handle_model.py): float64 numpy whose every value is a float32 number, so float32,
float64 and mixed-precision engines and the float64 oracle all see the same LP.  Importing this module needs no GPU; only
``HostLP.engine`` does."""
import numpy as np
import scipy.sparse as sp
import torch

from oracle import oracle as orc                                   # the checker (tests only)

DEV = "cuda:0"
NP = {torch.float32: np.float32, torch.float64: np.float64}


def _f32(v):
    return np.asarray(v, np.float32).astype(np.float64)


class HostLP:
    """``d_col`` / ``d_row``: the LP is the SCALED form of another one (K = D_row K_u D_col, c = D_col c_u, q = D_row q_u,
    l = l_u / D_col, u = u_u / D_col: enhancements.py:64-67), which ``unscaled=True`` passes evaluate (pdhg.py:157-161)"""

    def __init__(self, A, m_ineq, c, q, l, u, d_col=None, d_row=None):
        self.A = sp.csr_matrix(A, dtype=np.float64)
        self.A.sort_indices()
        self.m, self.n = self.A.shape
        self.m_ineq = int(m_ineq)
        self.c, self.q, self.l, self.u = (_f32(v) for v in (c, q, l, u))
        self.A.data = self.A.data.astype(np.float32).astype(np.float64)
        self.d_col = None if d_col is None else _f32(d_col)
        self.d_row = None if d_row is None else _f32(d_row)
        self._cache = {}

    def norm2(self):
        """||K||_2 by power iteration (float64, on the host)"""
        b = np.ones(self.n) / np.sqrt(max(self.n, 1))
        s = 0.0
        for _ in range(40):
            b = self.A.T @ (self.A @ b)
            s = np.linalg.norm(b)
            if s == 0:
                return 1.0
            b /= s
        return float(np.sqrt(s))

    def oracle(self, dtype):
        return orc.OracleLP(self.m, self.n, self.m_ineq, self.A.indptr, self.A.indices, self.A.data, self.c, self.q, self.l, self.u,
                            dtype=NP.get(dtype, dtype))

    def unscaled_oracle(self):
        """the float64 oracle of the un-preconditioned LP: evaluate it at (D_col x, D_row y)"""
        if "unscaled" not in self._cache:
            Ku = (sp.diags(1.0 / self.d_row) @ self.A @ sp.diags(1.0 / self.d_col)).tocsr()
            Ku.sort_indices()
            self._cache["unscaled"] = orc.OracleLP(self.m, self.n, self.m_ineq, Ku.indptr, Ku.indices, Ku.data, self.c / self.d_col,
                                                   self.q / self.d_row, self.l * self.d_col, self.u * self.d_col, dtype=np.float64)
        return self._cache["unscaled"]

    def engine(self, dtype, form="csr", tile_args=None, before_attach=None, **kw):
        """``tile_args``: for a tiled form, the ``build_tiles`` keywords of K and of K' (a pair of dicts: lw, rpt, groups, max_rest)
        in place of the default ``lw=6, rpt=1``; a side whose matrix cannot be tiled with them stays on the CSR kernel, and what the
        form says about groups and the remainder is then the caller's to assert.  ``before_attach(transpose, tiles)`` sees every
        tile set before the library does (which does not validate the format)."""
        import torchpdlp_amd as tp
        from torchpdlp_amd.tiled import build_tiles
        t = lambda v, dt=dtype: torch.tensor(np.asarray(v), dtype=dt, device=DEV)
        vec = kw.get("vec_dtype") or dtype
        if self.d_col is not None:
            kw = dict(kw, d_col=t(self.d_col, vec), d_row=t(self.d_row, vec))
        K = tp.CsrPair(self.m, self.n, t(self.A.indptr, torch.int32), t(self.A.indices, torch.int32), t(self.A.data))
        eng = tp.PdlpEngine.from_full(K, t(self.c, vec), t(self.q, vec), t(self.l, vec), t(self.u, vec), self.m_ineq, **kw)
        for tr in (0, 1):                       # (whatever the engine chose by itself for this shape: start from the CSR kernel)
            eng.attach_tiles(tr, None)
            eng.attach_sorted(tr, on=False)
        if form == "sorted":
            for tr in (0, 1):
                eng.attach_sorted(tr)
                assert "sorted" in eng.kernels[tr] or int((eng.KT if tr else eng.K)[2].numel()) == 0
        elif form != "csr":
            lim = eng.tile_limits()
            for tr, (rp, ci, va), rows, cols in ((0, eng.K, eng.ml, eng.n), (1, eng.KT, eng.nl, eng.m)):
                args = dict(lw=6, rpt=1, groups=2 if form == "tiles_groups" else 1) if tile_args is None else tile_args[tr]
                tl = build_tiles(rp, ci, va, rows, cols, max_groups=lim["max_groups"], kernel_limits=(lim["rpt_max"], lim["cap"], lim["nt"]),
                                 **args)
                if tile_args is not None:
                    if tl is not None:
                        if before_attach is not None:
                            before_attach(tr, tl)
                        eng.attach_tiles(tr, tl)
                    continue
                assert tl is not None, (form, tr)
                eng.attach_tiles(tr, tl)
                if form == "tiles_groups":
                    assert tl.groups == 2 and "2 groups" in eng.kernels[tr]
                if form == "tiles_remainder":
                    assert tl.nrem > 0 and "remainder" in eng.kernels[tr]
                else:
                    assert tl.nrem == 0
        return eng


def _bounds(rng, n, classes):
    l, u = np.full(n, -1.0), np.full(n, 2.0)
    if classes:
        l[::4], u[::4] = -np.inf, np.inf          # free
        l[1::4], u[1::4] = 0.5, 0.5               # fixed
        l[2::4] = -np.inf                         # upper only
        u[3::4] = np.inf                          # lower only
    return l, u


def edge_lp(case):
    """the five shapes of test_edge_cases_match_oracle (37 x 23; 1 x 1)"""
    rng = np.random.default_rng(21)
    if case == "one_by_one":
        m, n, m_ineq = 1, 1, 1
        Kd = np.array([[2.0]])
    else:
        m, n = 37, 23
        Kd = rng.standard_normal((m, n)) * (rng.random((m, n)) < 0.2)
        m_ineq = {"no_ineq": 0, "all_ineq": m}.get(case, 15)
        if case == "empty_row_and_col":
            Kd[5, :] = 0
            Kd[30, :] = 0
            Kd[:, 7] = 0
    l, u = _bounds(rng, n, case == "free_and_fixed")
    return HostLP(Kd, m_ineq, rng.standard_normal(n), rng.standard_normal(m), l, u)


def sparse_lp(m, n, per_row, seed, dense=False, scaled=False):
    """`per_row` entries in every row at random columns; `dense`: plus one full row and one full column; `scaled`: with D_col and
    D_row that are not ones (drawn after everything else: the LP itself is the one without them)"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(m), per_row)
    cols = rng.integers(0, n, size=m * per_row)
    A = sp.coo_matrix((rng.standard_normal(m * per_row), (rows, cols)), shape=(m, n)).tocsr()      # (duplicates are added up)
    if dense:
        A = A.tolil()
        A[m // 3, :] = rng.standard_normal(n)
        A[:, n // 2] = rng.standard_normal((m, 1))
        A = A.tocsr()
    l, u = _bounds(rng, n, True)
    c, q = rng.standard_normal(n), rng.standard_normal(m)
    d = dict(d_col=rng.uniform(0.5, 2.0, n), d_row=rng.uniform(0.5, 2.0, m)) if scaled else {}
    return HostLP(A, (2 * m) // 5, c, q, l, u, **d)


def sequence_lp():
    """400 x 300 for the call-sequence tests: all four bound classes, 160 inequality and 240 equality rows, one empty row (an
    inequality row) and one empty column, D_col and D_row in [0.5, 2]"""
    rng = np.random.default_rng(13)
    m, n, per_row = 400, 300, 6
    A = sp.coo_matrix((rng.standard_normal(m * per_row), (np.repeat(np.arange(m), per_row), rng.integers(0, n, size=m * per_row))),
                      shape=(m, n)).tolil()
    A[17, :] = 0
    A[:, 42] = 0
    l, u = _bounds(rng, n, True)
    return HostLP(A.tocsr(), 160, rng.standard_normal(n), rng.standard_normal(m), l, u, d_col=rng.uniform(0.5, 2.0, n),
                  d_row=rng.uniform(0.5, 2.0, m))


_LPS = {}


def get_lp(name):
    """built once per session, shared, never written to"""
    if name not in _LPS:
        _LPS[name] = (edge_lp(name[5:]) if name.startswith("edge_") else
                      {"mid": lambda: sparse_lp(600, 520, 8, 5), "mid_dense": lambda: sparse_lp(600, 520, 8, 6, dense=True),
                       "long": lambda: sparse_lp(2500, 2300, 3, 7, dense=True), "seq": sequence_lp,
                       "mid_scaled": lambda: sparse_lp(600, 520, 8, 5, scaled=True)}[name]())
    return _LPS[name]
