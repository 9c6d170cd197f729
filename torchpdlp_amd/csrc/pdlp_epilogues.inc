// pdlp_epilogues.inc -- epilogue functors: the PDHG half-steps, KKT sums and infeasibility tests fused into the products.
// Part of pdlp_hip.hip (included inside its anonymous namespace; not a translation unit of its own).
// ------------------------------------------------------------------------------------------------
// epilogues: called once per row with the row's dot product
// ------------------------------------------------------------------------------------------------
// Every epilogue also offers pre(row) / operator()(row, sum, pre, acc): the CSR kernel issues the row's operand loads
// (pre) together with the matrix loads, so they are off the dependent chain product -> epilogue.
struct NoPre {};

// Direct exchange (pdlp_peer_*, include/pdlp_hip.h): the block of a gathered vector that a half-step writes -- xbar, the new y, or their
// float32 differences in delta mode -- ALSO goes straight into the other ranks' copies of that vector, i.e. into their device memory
// opened over HIP IPC (xGMI between GPUs): the exchange rides on the product's own stores instead of following it as a collective.
// System-scope stores (written through, never left dirty in this GPU's L2); the flag that tells a peer its block is complete is stored
// by the NEXT kernel of the stream (k_peer_signal).  n = 0 (every handle outside pdlp_iterate's direct exchange): nothing happens.
// ON = false: an empty member -- the half-steps of every handle that is not inside the direct exchange run the instantiations
// without it (with the table as a run-time "n = 0" the single-GPU dual half-step measured 2 % slower: 1.763 against 1.720 ms).
template <typename T, bool ON> struct PeerOut {
    T* p[MAX_PEER];
    int n = 0;
    __device__ __forceinline__ void operator()(int j, T v) const
    {
#pragma unroll
        for (int q = 0; q < MAX_PEER; ++q)      // (static indices: the table stays in the kernel argument segment)
            if (q < n) __hip_atomic_store(p[q] + j, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
};
template <typename T> struct PeerOut<T, false> {
    __device__ __forceinline__ void operator()(int, T) const {}
};
template <typename T> struct StoreEpi {
    static constexpr int NA = 0;
    typedef NoPre Pre;
    T* out;
    __device__ void load() {}
    __device__ Pre pre(int) const { return Pre{}; }
    __device__ void operator()(int i, T s, double*) const { out[i] = s; }
    __device__ void operator()(int i, T s, const Pre&, double* a) const { (*this)(i, s, a); }
};

// Two-sided rows (pdlp_set_row_upper): q_i <= (K x)_i <= q_upper_i on the inequality rows.  RANGED = true adds ONE operand to the
// constraint-side functors -- q_upper[i], loaded in pre() beside q[i] -- and the upper side's arithmetic; RANGED = false (the default)
// has neither the pointer in the kernel arguments nor the value in the operand set (the tiled kernel sizes its epilogue groups by
// sizeof(Pre)), so those instantiations are what they were before two-sided rows existed.
// An operand that only the RANGED / QUAD form of a functor has: a T, or an empty member ([[no_unique_address]], last in the operand
// struct, so sizeof(Pre) is that of the members before it -- pinned by a static_assert beside each struct).
struct Absent {};
template <typename T, bool ON> using Opt = std::conditional_t<ON, T, Absent>;
template <typename T, bool RANGED> struct RowUpper {
    const T* p = nullptr;
    __device__ __forceinline__ T at(int i) const { return p[i]; }
};
template <typename T> struct RowUpper<T, false> {
    __device__ __forceinline__ Absent at(int) const { return {}; }
};
// y' of an inequality row from a = y + sigma (q - k) and b = y + sigma (q_upper - k): a above zero (the lower side pushes), b below
// zero (the upper side pushes), else 0.  Every operation is monotone, so a <= b after rounding too and at most one side is active.
// Written from a < 0 so that with q_upper = +inf (b = +inf) the value is the one-sided `a < 0 ? 0 : a` bit for bit (a = -0 included).
template <typename T> __device__ __forceinline__ T ranged_dual(T a, T b) { return a < (T)0 ? (b < (T)0 ? b : (T)0) : a; }

// Diagonal quadratic objective (pdlp_set_objective_diag): min c'x + 1/2 sum_j d_j x_j^2, d >= 0.  QUAD = true adds ONE operand to the
// variable-side functors -- d[j], loaded in pre() beside c[j] -- the division of the primal half-step's prox and the term d_j x_j of
// the gradient; QUAD = false (the default) has neither the pointer in the kernel arguments nor the value in the operand set (the tiled
// kernel sizes its epilogue groups by sizeof(Pre)), so those instantiations are what they were before the quadratic term existed.
// Only PEER = false functors have the QUAD form: a handle with the term is one GPU without an exchange.
template <typename T, bool QUAD> struct ObjDiag {
    const T* p = nullptr;
    __device__ __forceinline__ T at(int j) const { return p[j]; }
};
template <typename T> struct ObjDiag<T, false> {
    __device__ __forceinline__ Absent at(int) const { return {}; }
};
// the prox of tau (c'x + 1/2 x'Dx) at z = x - tau (c - K'y): z / (1 + tau d), before the clamp; d = 0 divides by 1, which is exact
template <typename T> __device__ __forceinline__ T quad_prox(T z, T tau, T dj) { return z / ((T)1 + tau * dj); }
// 1/2 d_j x_j^2 in double: joins c_j x_j in the primal objective's sum and leaves the sum l'max(lam, 0) of the dual objective.  Formed
// from the SCALED pair (d_s = d D_col^2, x_s = x / D_col), of which it is invariant, so UNSCALE needs no factor of its own.
template <typename T> __device__ __forceinline__ double quad_half(T dj, T xj) { return 0.5 * (double)dj * ((double)xj * (double)xj); }

// Sparse quadratic objective (pdlp_set_objective_matrix): min c'x + 1/2 x'Qx, Q symmetric positive semidefinite.  The prox of such an
// objective is not closed form, so the iteration takes the linearised step: the epilogue of the product Q x stores the gradient of
// the objective, g_j = c_j + (Q x)_j, and every variable-side functor then reads g where it reads c (the host swaps the pointer; no
// functor changes).  SUM (the KKT pass and the report): acc[0] takes x_j (Q x)_j in double, which finishes as x'Qx; the iteration's
// instantiation has no sum.  Over Q's own row blocks only (k_csr_fused / k_long_rows): Q has neither tiles nor a sorted copy.
template <typename T> struct ObjGradPre { T cj, xj; };
template <typename T, bool SUM> struct ObjGradEpi {
    static constexpr int NA = SUM ? 1 : 0;
    const T* c; const T* x; T* g;
    typedef ObjGradPre<T> Pre;
    __device__ void load() {}
    __device__ Pre pre(int j) const { return Pre{c[j], x[j]}; }
    __device__ void operator()(int j, T s, double* acc) const { (*this)(j, s, pre(j), acc); }
    __device__ void operator()(int j, T s, const Pre& p, double* acc) const
    {
        g[j] = p.cj + s;
        if (SUM) acc[0] += (double)p.xj * (double)s;
    }
};

// The same product behind the primal half-step of an adaptive iteration (pdlp_objective_iterate), taken at the NEW x: row j sees the
// gradient g_j of the old x, still in g[j] (the half-step that read it is an earlier launch; row j is the only reader and writer of
// g[j]), beside the one it forms, and the difference of the two is (Q dx)_j up to the rounding of either.  acc[0] takes
// dx_j (g'_j - g_j) in double, g' the STORED value: the sum finishes as the curvature dx'Q dx of the step-size rule without a
// product of its own.  The cancellation in g' - g is of order eps |g| |dx| per row (DESIGN.md 4.5.1).  Q's own row blocks only.
template <typename T> struct ObjGradStepPre { T cj, xn, xo, go; };
template <typename T> struct ObjGradStepEpi {
    static constexpr int NA = 1;
    const T* c; const T* x_new; const T* x_old; T* g;
    typedef ObjGradStepPre<T> Pre;
    __device__ void load() {}
    __device__ Pre pre(int j) const { return Pre{c[j], x_new[j], x_old[j], g[j]}; }
    __device__ void operator()(int j, T s, double* acc) const { (*this)(j, s, pre(j), acc); }
    __device__ void operator()(int j, T s, const Pre& p, double* acc) const
    {
        const T gn = p.cj + s;
        g[j] = gn;
        acc[0] += (double)(p.xn - p.xo) * ((double)gn - (double)p.go);
    }
};

// ---- the arithmetic every kernel file shares (this file is included before all of them) --------------------------------------
// lam = project_lambda_box(g) (helpers.py:21-37) with the bound classes read off l, u: a variable without a lower bound takes
// min(g, 0), one without an upper bound max(g, 0), a free one 0, a boxed one g.  ninf / pinf: the classes, for the callers' own use.
// (Operands by reference here and in primal_step: handed over by value the compiler knows them to be defined and folds the `&&`
// otherwise than in a body written out; by reference the kernels are what they were, instruction for instruction.)
template <typename T> __device__ __forceinline__ T project_lambda(const T& g, const bool& ninf, const bool& pinf)
{
    T lam;
    if (ninf && pinf) lam = (T)0;
    else if (ninf) lam = g < (T)0 ? g : (T)0;
    else if (pinf) lam = g > (T)0 ? g : (T)0;
    else lam = g;
    return lam;
}
template <typename T> struct BoxLam { T lam; bool ninf, pinf; };
template <typename T> __device__ __forceinline__ BoxLam<T> project_lambda(const T& g, const T& lo, const T& hi)
{
    const bool ninf = isinf(lo) && lo < (T)0, pinf = isinf(hi) && hi > (T)0;
    return {project_lambda(g, ninf, pinf), ninf, pinf};
}
// x' = clamp(x - tau (c - K'y), l, u) (step.py:25-30 / :74-82; PDHG_step spectral_casting.py:277-284), with the prox of the
// quadratic term ahead of the clamp when there is a d_j
template <typename T, bool QUAD = false>
__device__ __forceinline__ T primal_step(const T& xo, const T& tau, const T& cj, const T& kty, const T& lo, const T& hi, const Opt<T, QUAD>& dj = {})
{
    const T grad = cj - kty;
    T v = xo - tau * grad;
    if constexpr (QUAD) v = quad_prox(v, tau, dj);
    v = v < lo ? lo : v;
    v = v > hi ? hi : v;
    return v;
}
// y' = y + sigma (q - K xbar), an inequality row (i < ineq_end) projected onto y >= 0 (step.py:33-38 / :85-90; PDHG_step
// spectral_casting.py:287-292).  The RANGED form of DualEpi and HalpernDualEpi projects with ranged_dual in the functor's own body:
// through this function the tiled kernel of those two comes out with selects where it has branches.
template <typename T> __device__ __forceinline__ T dual_step(int i, int ineq_end, T yo, T sigma, T qi, T k)
{
    T v = yo + sigma * (qi - k);
    if (i < ineq_end && v < (T)0) v = (T)0;
    return v;
}

// primal half-step over this rank's rows of K' (= its variables).  kty = (K'y)_j.
// step.py:25-30 (fixed) / :74-82 (adaptive); running sum pdhg.py:107.
template <typename T, bool QUAD> struct PrimalPre { T xo, cj, lo, hi, sum, ks; [[no_unique_address]] Opt<T, QUAD> dj; };
static_assert(sizeof(PrimalPre<float, false>) == 6 * 4 && sizeof(PrimalPre<double, true>) == 7 * 8, "operands only");
template <typename T, bool ADAPT, bool PEER = false, bool QUAD = false> struct PrimalEpi {
    static_assert(!(QUAD && PEER), "the quadratic term has no sharded form");
    static constexpr int NA = ADAPT ? 1 : 0;
    const T* x_old; T* x_new; T* xbar; const T* c; const T* l; const T* u; T* x_sum; const double* sc;
    // kty_sum (or null): running sum of w_k K'y_k -- K'y of the averaged iterate without a product at the restart check.  The
    // product of this half-step is K'y of the PREVIOUS iterate's y (weight w_pending when adaptive, eta when fixed: the
    // host passes null for the first half-step after a restart, whose y is the restart point and not part of the average)
    T* kty_sum = nullptr;
    T tau = 0, theta = 0, w = 0, wk = 0;
    PeerOut<T, PEER> peer{};               // the other ranks' xbar, at this rank's block
    [[no_unique_address]] ObjDiag<T, QUAD> diag{};          // d of this rank's variables
    static constexpr bool working_matrix_only = QUAD;      // (launch_csr)
    __device__ void load()
    {
        tau = (T)sc[S_TAU];
        theta = (T)sc[S_THETA];
        w = ADAPT ? (T)sc[S_WPEND] : (T)sc[S_ETA];
        wk = w;
    }
    typedef PrimalPre<T, QUAD> Pre;
    __device__ Pre pre(int j) const
    {
        return Pre{x_old[j], c[j], l[j], u[j], x_sum[j], kty_sum ? kty_sum[j] : (T)0, diag.at(j)};
    }
    __device__ void operator()(int j, T kty, double* acc) const { (*this)(j, kty, pre(j), acc); }
    __device__ void operator()(int j, T kty, const Pre& p, double* acc) const
    {
        const T xo = p.xo;
        if (kty_sum) kty_sum[j] = p.ks + wk * kty;
        const T v = primal_step<T, QUAD>(xo, tau, p.cj, kty, p.lo, p.hi, p.dj);
        const T d = v - xo;
        x_new[j] = v;
        const T xb = v + theta * d;
        xbar[j] = xb;
        peer(j, xb);
        if (ADAPT) {
            x_sum[j] = p.sum + w * xo;    // weight of the PREVIOUS iterate, known only now
            acc[0] += (double)d * (double)d;
        } else {
            x_sum[j] = p.sum + w * v;
        }
    }
};

// dual half-step over this rank's rows of K (= its constraints).  kxbar = (K xbar)_i.
// step.py:33-38 / :85-96; running sum pdhg.py:108.
template <typename T, bool RANGED> struct DualPre { T yo, qi, sum, kxo, kxs; [[no_unique_address]] Opt<T, RANGED> qu; };
static_assert(sizeof(DualPre<float, false>) == 5 * 4 && sizeof(DualPre<double, true>) == 6 * 8, "operands only");
template <typename T, bool ADAPT, bool PEER = false, bool RANGED = false> struct DualEpi {
    static constexpr int NA = ADAPT ? 2 : 0;
    const T* y_old; T* y_new; const T* q; T* y_sum; T* kx; const double* sc; int ineq_end;
    // kx: K x of the current iterate, carried along (K x+ = K x + (K xbar - K x)/(1 + theta)); kx_sum (or null): running sum of
    // w_k K x_k -- K x of the averaged iterate without a product at the restart check
    T* kx_sum = nullptr;
    T sigma = 0, w = 0, inv1pt = 0;
    PeerOut<T, PEER> peer{};               // the other ranks' copy of the y buffer being written, at this rank's block
    [[no_unique_address]] RowUpper<T, RANGED> upper{};      // q_upper of this rank's rows
    static constexpr bool working_matrix_only = RANGED;
    __device__ void load()
    {
        sigma = (T)sc[S_SIGMA];
        w = ADAPT ? (T)sc[S_WPEND] : (T)sc[S_ETA];
        inv1pt = (T)sc[S_INV1PT];
    }
    typedef DualPre<T, RANGED> Pre;
    __device__ Pre pre(int i) const
    {
        return Pre{y_old[i], q[i], y_sum[i], kx[i], kx_sum ? kx_sum[i] : (T)0, upper.at(i)};
    }
    __device__ void operator()(int i, T kxbar, double* acc) const { (*this)(i, kxbar, pre(i), acc); }
    __device__ void operator()(int i, T kxbar, const Pre& p, double* acc) const
    {
        const T yo = p.yo;
        T v;
        if constexpr (RANGED) {
            v = yo + sigma * (p.qi - kxbar);
            if (i < ineq_end) v = ranged_dual(v, yo + sigma * (p.qu - kxbar));
        } else {
            v = dual_step(i, ineq_end, yo, sigma, p.qi, kxbar);
        }
        y_new[i] = v;
        peer(i, v);
        // K dx = (K xbar - K x) / (1 + theta) because xbar = x + (1 + theta) dx; kx caches K x
        const T kxo = p.kxo;
        const T kdx = (kxbar - kxo) * inv1pt;
        const T kxn = kxo + kdx;
        kx[i] = kxn;
        if (ADAPT) {
            y_sum[i] = p.sum + w * yo;                      // weight of the PREVIOUS iterate, known only now
            if (kx_sum) kx_sum[i] = p.kxs + w * kxo;
            const T dy = v - yo;
            acc[0] += (double)dy * (double)dy;
            acc[1] += (double)dy * (double)kdx;
        } else {
            y_sum[i] = p.sum + w * v;
            if (kx_sum) kx_sum[i] = p.kxs + w * kxn;
        }
    }
};

// Reflected Halpern iteration (pdlp_halpern_iterate; the reference has no counterpart), primal half over the rows of K'.
// x' and xbar are formed with PrimalEpi's own expressions at theta = 1 (the candidate equals one fixed PDHG step bit for bit);
// the new iterate is the reflected point xbar = 2x' - x pulled towards the anchor: x+ = a xbar + b x_last, a = (t+1)/(t+2),
// b = 1/(t+2) rounded once on the host.  No running sums: five operand loads, three stores.
template <typename T, bool QUAD> struct HalpernPrimalPre { T xo, xl, cj, lo, hi; [[no_unique_address]] Opt<T, QUAD> dj; };
static_assert(sizeof(HalpernPrimalPre<float, false>) == 5 * 4 && sizeof(HalpernPrimalPre<double, true>) == 6 * 8, "operands only");
template <typename T, bool QUAD = false> struct HalpernPrimalEpi {
    static constexpr int NA = 0;
    const T* x_old; T* x_new; T* xbar; T* x_cand; const T* x_last; const T* c; const T* l; const T* u; const double* sc;
    T a, b;
    T tau = 0;
    [[no_unique_address]] ObjDiag<T, QUAD> diag{};
    static constexpr bool working_matrix_only = QUAD;
    __device__ void load() { tau = (T)sc[S_TAU]; }
    typedef HalpernPrimalPre<T, QUAD> Pre;
    __device__ Pre pre(int j) const
    {
        return Pre{x_old[j], x_last[j], c[j], l[j], u[j], diag.at(j)};
    }
    __device__ void operator()(int j, T kty, double* acc) const { (*this)(j, kty, pre(j), acc); }
    __device__ void operator()(int j, T kty, const Pre& p, double*) const
    {
        const T xo = p.xo;
        const T v = primal_step<T, QUAD>(xo, tau, p.cj, kty, p.lo, p.hi, p.dj);
        const T d = v - xo;
        x_cand[j] = v;
        const T xb = v + d;                // (PrimalEpi's v + theta * d at theta = 1: the product with 1 is exact)
        xbar[j] = xb;
        x_new[j] = a * xb + b * p.xl;
    }
};

// Reflected Halpern iteration, dual half over the rows of K: y' as DualEpi forms it; y+ = a (2y' - y) + b y_last.
template <typename T, bool RANGED> struct HalpernDualPre { T yo, yl, qi; [[no_unique_address]] Opt<T, RANGED> qu; };
static_assert(sizeof(HalpernDualPre<float, false>) == 3 * 4 && sizeof(HalpernDualPre<double, true>) == 4 * 8, "operands only");
template <typename T, bool RANGED = false> struct HalpernDualEpi {
    static constexpr int NA = 0;
    const T* y_old; T* y_new; T* y_cand; const T* y_last; const T* q; const double* sc; int ineq_end;
    T a, b;
    T sigma = 0;
    [[no_unique_address]] RowUpper<T, RANGED> upper{};
    static constexpr bool working_matrix_only = RANGED;
    __device__ void load() { sigma = (T)sc[S_SIGMA]; }
    typedef HalpernDualPre<T, RANGED> Pre;
    __device__ Pre pre(int i) const
    {
        return Pre{y_old[i], y_last[i], q[i], upper.at(i)};
    }
    __device__ void operator()(int i, T kxbar, double* acc) const { (*this)(i, kxbar, pre(i), acc); }
    __device__ void operator()(int i, T kxbar, const Pre& p, double*) const
    {
        const T yo = p.yo;
        T v;
        if constexpr (RANGED) {
            v = yo + sigma * (p.qi - kxbar);
            if (i < ineq_end) v = ranged_dual(v, yo + sigma * (p.qu - kxbar));
        } else {
            v = dual_step(i, ineq_end, yo, sigma, p.qi, kxbar);
        }
        y_cand[i] = v;
        y_new[i] = a * ((T)2 * v - yo) + b * p.yl;
    }
};

// Fixed-point residual of the Halpern iteration (pdlp_halpern_fixed_point), over the rows of K' with ktdy = (K'dy)_j, dy = y - y' the
// gathered vector: dx = x_prev - x_cand, acc[0] = sum dx^2, acc[1] = sum (K'dy)_j dx_j.  Two operand loads, no store.
template <typename T> struct FixedPointPre { T xp, xc; };
template <typename T> struct FixedPointEpi {
    static constexpr int NA = 2;
    const T* x_prev; const T* x_cand;
    typedef FixedPointPre<T> Pre;
    __device__ void load() {}
    __device__ Pre pre(int j) const { return Pre{x_prev[j], x_cand[j]}; }
    __device__ void operator()(int j, T ktdy, double* acc) const { (*this)(j, ktdy, pre(j), acc); }
    __device__ void operator()(int, T ktdy, const Pre& p, double* acc) const
    {
        const T dx = p.xp - p.xc;
        acc[0] += (double)dx * (double)dx;
        acc[1] += (double)ktdy * (double)dx;
    }
};

// KKT, dual side (helpers.py:75-84,94 with project_lambda_box helpers.py:21-37 and pdhg.py:11-17)
// Quadratic term (QUAD): the gradient is g = c + d x - K'y (formed from the scaled operands, before UNSCALE divides it), the primal
// objective's sum acc[3] takes c_j x_j + 1/2 d_j x_j^2 and acc[1] takes -1/2 d_j x_j^2 besides l'max(lam, 0): the dual objective of the
// quadratic problem is q'y + l'lam+ + u'lam- - 1/2 x'Dx, and the six sums keep their places (include/pdlp_hip.h).
template <typename T, bool QUAD> struct KktDualPre { T cj, lo, hi, xj, d; [[no_unique_address]] Opt<T, QUAD> qd; };
static_assert(sizeof(KktDualPre<float, false>) == 5 * 4 && sizeof(KktDualPre<double, true>) == 6 * 8, "operands only");
// the four sums of a variable from (K'y)_j and its operands -- the counterpart of row_sums, shared by the KKT pass and the report;
// KEEP: lam_j goes to lam_out[j] (UNSCALE: of the un-preconditioned problem)
template <typename T, bool UNSCALE, bool QUAD, bool KEEP = false>
__device__ __forceinline__ void col_sums(T kty, const KktDualPre<T, QUAD>& p, double* acc, T* lam_out = nullptr, int j = 0)
{
    T cj = p.cj, lo = p.lo, hi = p.hi, xj = p.xj;
    T g = cj - kty;
    [[maybe_unused]] double hq = 0.0;
    if constexpr (QUAD) g = (cj + p.qd * xj) - kty;
    if (UNSCALE) {            // K_u'(D_row y) = (K_s'y)/D_col, c_u = c_s/D_col, l_u = l_s D_col, x_u = D_col x
        const T d = p.d;
        g = g / d; cj = cj / d; lo = lo * d; hi = hi * d; xj = xj * d;
    }
    if constexpr (QUAD) hq = quad_half(p.qd, p.xj);         // (of the scaled pair)
    const BoxLam<T> b = project_lambda(g, lo, hi);
    const T lam = b.lam;
    if constexpr (KEEP) lam_out[j] = lam;
    const T ld = b.ninf ? (T)0 : lo, ud = b.pinf ? (T)0 : hi;
    const T r = g - lam;
    acc[0] += (double)r * (double)r;
    acc[1] += (double)ld * (double)(lam > (T)0 ? lam : (T)0);
    acc[2] += (double)ud * (double)(lam < (T)0 ? lam : (T)0);
    acc[3] += (double)cj * (double)xj;
    if constexpr (QUAD) { acc[1] -= hq; acc[3] += hq; }     // (own additions: with d = 0 the sums are the linear ones bit for bit)
}
template <typename T, bool UNSCALE, bool QUAD = false> struct KktDualEpi {
    static constexpr int NA = 4;
    const T* x; const T* c; const T* l; const T* u; const T* dcol; T* kty_out;     // kty_out: keeps K'y for the next primal half-step
    [[no_unique_address]] ObjDiag<T, QUAD> diag{};
    static constexpr bool working_matrix_only = QUAD;
    __device__ void load() {}
    typedef KktDualPre<T, QUAD> Pre;
    __device__ Pre pre(int j) const { return Pre{c[j], l[j], u[j], x[j], UNSCALE ? dcol[j] : (T)1, diag.at(j)}; }
    __device__ void operator()(int j, T kty, double* acc) const { (*this)(j, kty, pre(j), acc); }
    __device__ void operator()(int j, T kty, const Pre& p, double* acc) const
    {
        if (kty_out) kty_out[j] = kty;
        col_sums<T, UNSCALE, QUAD>(kty, p, acc);
    }
};

// KKT, primal side (helpers.py:77,87-91).  Optionally keeps K x for the adaptive step's cache.
// Two-sided rows (RANGED): the upper violation max(k - q_upper, 0) joins the lower one min(k - q, 0) in acc[0] (0 for +inf), and the
// dual objective takes q_upper_i y_i where y_i < 0 on a row with a finite q_upper (the upper side is the active one).
template <typename T, bool RANGED> struct KktPrimalPre { T qi, yi, d; [[no_unique_address]] Opt<T, RANGED> qu; };
static_assert(sizeof(KktPrimalPre<float, false>) == 3 * 4 && sizeof(KktPrimalPre<double, true>) == 4 * 8, "operands only");
// the two sums of a constraint row from r = k - q and ru = k - q_upper (RANGED), after UNSCALE has divided them
template <typename T, bool RANGED>
__device__ __forceinline__ void row_sums(int i, int ineq_end, T r, T ru, T qi, T qu, T yi, double* acc)
{
    if (i < ineq_end && r > (T)0) r = (T)0;
    acc[0] += (double)r * (double)r;
    if constexpr (RANGED) {
        if (i < ineq_end) {
            ru = ru > (T)0 ? ru : (T)0;
            acc[0] += (double)ru * (double)ru;
            if (yi < (T)0 && !isinf(qu)) qi = qu;
        }
    }
    acc[1] += (double)qi * (double)yi;
}
template <typename T, bool UNSCALE, bool RANGED = false> struct KktPrimalEpi {
    static constexpr int NA = 2;
    const T* y; const T* q; const T* drow; T* kx_out; int ineq_end;
    [[no_unique_address]] RowUpper<T, RANGED> upper{};
    static constexpr bool working_matrix_only = RANGED;
    __device__ void load() {}
    typedef KktPrimalPre<T, RANGED> Pre;
    __device__ Pre pre(int i) const
    {
        return Pre{q[i], y[i], UNSCALE ? drow[i] : (T)1, upper.at(i)};
    }
    __device__ void operator()(int i, T kx, double* acc) const { (*this)(i, kx, pre(i), acc); }
    __device__ void operator()(int i, T kx, const Pre& p, double* acc) const
    {
        if (kx_out) kx_out[i] = kx;
        T qi = p.qi, yi = p.yi, qu = (T)0, ru = (T)0;
        T r = kx - qi;
        if constexpr (RANGED) { qu = p.qu; ru = kx - qu; }
        if (UNSCALE) {            // K_u (D_col x) = (K_s x)/D_row, q_u = q_s/D_row, y_u = D_row y
            const T d = p.d;
            r = r / d; qi = qi / d; yi = yi * d;
            if constexpr (RANGED) { ru = ru / d; qu = qu / d; }
        }
        row_sums<T, RANGED>(i, ineq_end, r, ru, qi, qu, yi, acc);
    }
};

// Solution report, variable side (pdlp_report_local): the vector pass that follows a plain product K'y stored into `buf`.  Reads
// (K'y)_j from buf, forms the sums of KktDualEpi with the same arithmetic (helpers.py:75-84,94; project_lambda_box helpers.py:21-37)
// and leaves the reduced cost lam_j in buf[j] -- UNSCALE: of the un-preconditioned problem, lam_u = lam_s / D_col (pdhg.py:157-161).
// The product is an operand of pre(), not the kernel's row sum (k_rowsum_epilogue runs with no groups): buf is read and written
// through this one pointer.
template <typename T, bool UNSCALE, bool QUAD = false> struct ReportDualEpi {
    static constexpr int NA = 4;
    T* buf; const T* x; const T* c; const T* l; const T* u; const T* dcol;
    [[no_unique_address]] ObjDiag<T, QUAD> diag{};
    __device__ void load() {}
    struct Pre { T kty; KktDualPre<T, QUAD> kp; };
    __device__ Pre pre(int j) const { return Pre{buf[j], {c[j], l[j], u[j], x[j], UNSCALE ? dcol[j] : (T)1, diag.at(j)}}; }
    __device__ void operator()(int j, T, double* acc) const { (*this)(j, (T)0, pre(j), acc); }
    __device__ void operator()(int j, T, const Pre& p, double* acc) const { col_sums<T, UNSCALE, QUAD, true>(p.kty, p.kp, acc, buf, j); }
};

// Solution report, constraint side: the same after K x stored into `buf`.  The sums of KktPrimalEpi (helpers.py:77,87-91); buf[i]
// keeps the row activity (K x)_i -- UNSCALE: act_u = (K_s x_s) / D_row.
template <typename T, bool RANGED> struct ReportPrimalPre { T kx, qi, yi, d; [[no_unique_address]] Opt<T, RANGED> qu; };
static_assert(sizeof(ReportPrimalPre<float, false>) == 4 * 4 && sizeof(ReportPrimalPre<double, true>) == 5 * 8, "operands only");
template <typename T, bool UNSCALE, bool RANGED = false> struct ReportPrimalEpi {
    static constexpr int NA = 2;
    T* buf; const T* y; const T* q; const T* drow; int ineq_end;
    [[no_unique_address]] RowUpper<T, RANGED> upper{};
    __device__ void load() {}
    typedef ReportPrimalPre<T, RANGED> Pre;
    __device__ Pre pre(int i) const
    {
        return Pre{buf[i], q[i], y[i], UNSCALE ? drow[i] : (T)1, upper.at(i)};
    }
    __device__ void operator()(int i, T, double* acc) const { (*this)(i, (T)0, pre(i), acc); }
    __device__ void operator()(int i, T, const Pre& p, double* acc) const
    {
        T qi = p.qi, yi = p.yi, qu = (T)0, ru = (T)0;
        T r = p.kx - qi;
        if constexpr (RANGED) { qu = p.qu; ru = p.kx - qu; }
        if (UNSCALE) {
            const T d = p.d;
            r = r / d; qi = qi / d; yi = yi * d;
            buf[i] = p.kx / d;
            if constexpr (RANGED) { ru = ru / d; qu = qu / d; }
        }
        row_sums<T, RANGED>(i, ineq_end, r, ru, qi, qu, yi, acc);
    }
};

// infeasibility detection (opt-in), variable side -- detect_infeasibility enhancements.py:108-114,124-139,146-157 for
// the step just taken, with lam = project_lambda_box(c - K'y) (pdhg.py:90, helpers.py:21-37).  Rows of K'.
// partial sums: ||K'dy - dlam||^2, l_f'dlam_minus + u_f'dlam_plus, c'dx, #{variables failing the bound test}
template <typename T> struct InfeasDualEpi {
    static constexpr int NA = 4;
    const T* x; const T* x_prev; const T* c; const T* l; const T* u; const T* ktdy; T* lam_prev; T tol;
    typedef NoPre Pre;
    __device__ void load() {}
    __device__ Pre pre(int) const { return Pre{}; }
    __device__ void operator()(int j, T kty, const Pre&, double* acc) const { (*this)(j, kty, acc); }
    __device__ void operator()(int j, T kty, double* acc) const
    {
        const T cj = c[j], lo = l[j], hi = u[j];
        const T g = cj - kty;
        // (the classes formed here and not by project_lambda(g, lo, hi): isinf(lo) and isinf(hi) are read again below, and with the
        // classes folded inside the shared function this functor's kernels come out with other instructions)
        const bool ninf = isinf(lo) && lo < (T)0, pinf = isinf(hi) && hi > (T)0;
        const T lam = project_lambda(g, ninf, pinf);
        const T dlam = lam - lam_prev[j];                                    // :110
        lam_prev[j] = lam;                                                   // pdhg.py:101
        const T r = ktdy[j] - dlam;                                          // :146
        acc[0] += (double)r * (double)r;
        const T plus = -dlam > (T)0 ? -dlam : (T)0, minus = dlam > (T)0 ? dlam : (T)0;   // :113-114
        double lu = 0.0;
        if (!isinf(lo) && lo != (T)0) lu += (double)lo * (double)minus;      // :151,155
        if (!isinf(hi) && hi != (T)0) lu += (double)hi * (double)plus;       // :152,157
        acc[1] += lu;
        const T d = x[j] - x_prev[j];                                        // :108
        acc[2] += (double)cj * (double)d;                                    // :124
        const T ad = d < (T)0 ? -d : d;
        const bool ok = (!isinf(lo) && !isinf(hi) && ad <= tol) || (pinf && cj >= (T)0 && d >= -tol) ||
                        (ninf && cj <= (T)0 && d <= tol);                    // :135-137
        acc[3] += ok ? 0.0 : 1.0;
    }
};

// infeasibility detection, constraint side (rows of K): kdx = (K dx)_i.  enhancements.py:118,121,148-149
// partial sums: ||K_eq dx||^2, #{(K_in dx)_i < -tol}, #{dy_i < -tol, i inequality}, q'dy
template <typename T> struct InfeasPrimalEpi {
    static constexpr int NA = 4;
    const T* y; const T* y_prev; const T* q; T tol; int ineq_end;
    typedef NoPre Pre;
    __device__ void load() {}
    __device__ Pre pre(int) const { return Pre{}; }
    __device__ void operator()(int i, T kdx, const Pre&, double* acc) const { (*this)(i, kdx, acc); }
    __device__ void operator()(int i, T kdx, double* acc) const
    {
        const T dy = y[i] - y_prev[i];                                       // :109
        if (i < ineq_end) {
            acc[1] += (kdx >= -tol) ? 0.0 : 1.0;
            acc[2] += (dy >= -tol) ? 0.0 : 1.0;
        } else {
            acc[0] += (double)kdx * (double)kdx;
        }
        acc[3] += (double)q[i] * (double)dy;
    }
};

// ------------------------------------------------------------------------------------------------
// delta mode (mixed precision: float32 matrix, float64 vectors).  The product the kernel hands over is a float32 sum over a
// float32 DIFFERENCE vector; it is added to a float64 anchor product carried along (K'y resp. K x of the current iterate).
// Rounding then scales with the size of the step, not with the size of the iterate: the error of K'y_new is
// eps32 ||K|| ||dy|| on top of the anchor's, and the anchors are recomputed exactly (float64 accumulation) at every restart.
// ------------------------------------------------------------------------------------------------
// primal half-step: kty = KTY + K'(dy_f32); x+ = clamp(x - tau (c - kty), l, u); gdx = float(x+ - x) for the dual half-step.
// step.py:25-30 / :74-82 in exact arithmetic; running sum pdhg.py:107.
template <bool ADAPT, bool PEER = false> struct DeltaPrimalEpi {
    static constexpr int NA = ADAPT ? 1 : 0;
    const double* x_old; double* x_new; float* gdx; const double* c; const double* l; const double* u; double* x_sum; double* kty;
    const double* sc;
    double tau = 0, w = 0;
    PeerOut<float, PEER> peer{};           // the other ranks' gdx, at this rank's block
    __device__ void load()
    {
        tau = sc[S_TAU];
        w = ADAPT ? sc[S_WPEND] : sc[S_ETA];
    }
    struct Pre { double xo, cj, lo, hi, sum, ky; };
    __device__ Pre pre(int j) const { return Pre{x_old[j], c[j], l[j], u[j], x_sum[j], kty[j]}; }
    __device__ void operator()(int j, float s, double* acc) const { (*this)(j, s, pre(j), acc); }
    __device__ void operator()(int j, float s, const Pre& p, double* acc) const
    {
        const double ky = p.ky + (double)s;
        kty[j] = ky;
        const double xo = p.xo;
        const double v = primal_step(xo, tau, p.cj, ky, p.lo, p.hi);
        const double d = v - xo;
        x_new[j] = v;
        gdx[j] = (float)d;
        peer(j, (float)d);
        if (ADAPT) {
            x_sum[j] = p.sum + w * xo;
            acc[0] += d * d;
        } else {
            x_sum[j] = p.sum + w * v;
        }
    }
};

// dual half-step: K xbar = KX + (1 + theta) K(dx_f32) because xbar = x + (1 + theta) dx; KX <- KX + K dx; gdy = float(y+ - y).
// step.py:33-38 / :85-96; running sum pdhg.py:108.
template <bool ADAPT, bool PEER = false> struct DeltaDualEpi {
    static constexpr int NA = ADAPT ? 2 : 0;
    const double* y_old; double* y_new; float* gdy; const double* q; double* y_sum; double* kx; const double* sc; int ineq_end;
    double sigma = 0, w = 0, onept = 0;
    PeerOut<float, PEER> peer{};           // the other ranks' gdy, at this rank's block
    __device__ void load()
    {
        sigma = sc[S_SIGMA];
        w = ADAPT ? sc[S_WPEND] : sc[S_ETA];
        onept = 1.0 + sc[S_THETA];
    }
    struct Pre { double yo, qi, sum, kxo; };
    __device__ Pre pre(int i) const { return Pre{y_old[i], q[i], y_sum[i], kx[i]}; }
    __device__ void operator()(int i, float s, double* acc) const { (*this)(i, s, pre(i), acc); }
    __device__ void operator()(int i, float s, const Pre& p, double* acc) const
    {
        const double kdx = (double)s;
        const double yo = p.yo;
        const double v = dual_step(i, ineq_end, yo, sigma, p.qi, p.kxo + onept * kdx);
        y_new[i] = v;
        const double dy = v - yo;
        gdy[i] = (float)dy;
        peer(i, (float)dy);
        kx[i] = p.kxo + kdx;
        if (ADAPT) {
            y_sum[i] = p.sum + w * yo;
            acc[0] += dy * dy;
            acc[1] += dy * kdx;
        } else {
            y_sum[i] = p.sum + w * v;
        }
    }
};

// anchor + float32 product handed to a float64 epilogue (the KKT sums of a candidate): inner(row, anchor[row] + s).
// FOLD: the anchor itself advances to the sum (K'y of the current iterate once its pending dy is folded in).
template <class Inner, bool FOLD> struct AnchorEpi {
    static constexpr int NA = Inner::NA;
    Inner inner; double* anchor;
    __device__ void load() { inner.load(); }
    struct Pre { typename Inner::Pre ip; double a; };
    __device__ Pre pre(int r) const { return Pre{inner.pre(r), anchor[r]}; }
    __device__ void operator()(int r, float s, double* acc) const { (*this)(r, s, pre(r), acc); }
    __device__ void operator()(int r, float s, const Pre& p, double* acc) const
    {
        const double v = p.a + (double)s;
        if (FOLD) anchor[r] = v;
        inner(r, v, p.ip, acc);
    }
};

// anchor += float32 product (nothing else)
struct FoldEpi {
    static constexpr int NA = 0;
    double* anchor;
    typedef NoPre Pre;
    __device__ void load() {}
    __device__ Pre pre(int) const { return Pre{}; }
    __device__ void operator()(int r, float s, double*) const { anchor[r] += (double)s; }
    __device__ void operator()(int r, float s, const Pre&, double* a) const { (*this)(r, s, a); }
};
