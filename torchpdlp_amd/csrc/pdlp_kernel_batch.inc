// pdlp_kernel_batch.inc -- batched solves: B LPs over ONE constraint matrix, or one matrix each over one shared pattern, advanced
// together (pdlp_batch_*).
// Part of pdlp_hip.hip (included inside its anonymous namespace; not a translation unit of its own).
//
// Populations are row-major V[row][Bp]: column b is LP b, Bp is B rounded up to a multiple of the group width W (8, 16, 32).
// A launch has gridDim.y = Bp / W; group g serves columns [g W, (g + 1) W).  One product kernel, k_batch_mv<T, W, PERLP, Sel, Epi>:
// a selector (BSelLive, BSelAll, BSelList) says which columns take part, an epilogue what happens to a row's sum.  Inside a wave, W lanes work on a row
// (lane % W = the LP of the group), 64 / W rows at a time, each lane walking the row's items in CSR order -- the row walk of
// k_csr_mv: an item reads one coalesced segment of W values of the gathered population.
//
// Determinism: no atomics.  Per-LP sums go through fixed-order partials: lanes of equal LP over a wave (xor tree), then the
// four waves, then the blocks in a fixed tree (batch_block_sum: one workgroup per sum).  gridDim.x is a function of the row
// count and W only, so an LP's
// arithmetic does not depend on B, on its position in the batch or on the other LPs.
//
// Per-LP matrices (PERLP): the LPs share the pattern (row pointers, column indices) and each has its own values, a population
// vaB[nnz][Bp] like every other: item p of column b is vaB[p * Bp + b] (64-bit index), so the W lanes of a row read one contiguous
// segment per item, as the gather does, and the summation order of a row is the shared-matrix one.  Without the flag the kernels
// are the shared-matrix code unchanged.  The Ruiz factors are then per LP as well (dcol[n][Bp], drow[m][Bp]: `dper` of the
// un-scaling epilogues).
//
// Per-LP device scalars (working precision, [Bp]): eta (the step of the next iteration), omega, eta_sum (of the running
// average), wpend (adaptive: the weight of the current iterate, added to the sums by the next iteration); live[Bp] (int32):
// a column with live == 0 is frozen -- no kernel stores into it.
// ------------------------------------------------------------------------------------------------
constexpr int BATCH_MAXG = 8192;      // workgroups per group of columns at most (partials: BATCH_MAXG x Bp x 4 doubles per set)

inline int batch_grid(int64_t rows, int W)
{
    const int64_t rpb = (int64_t)(BLOCK / 64) * (64 / W);
    const int64_t g = (rows + rpb - 1) / rpb;
    return (int)(g < 1 ? 1 : (g > BATCH_MAXG ? BATCH_MAXG : g));
}

// column `b` of a vector that is either shared ([len], per = 0) or one column per LP ([len][Bp], per = 1)
#define BCOL(ptr, per, r, at) ((ptr)[(per) ? (at) : (size_t)(r)])

// partials[block][column][NA], column = blockIdx.y * W + lane
template <int W, int NA> __device__ __forceinline__ void batch_store_partials(const double* acc, double* partials, int Bp)
{
    __shared__ double red[BLOCK / 64][W][NA > 0 ? NA : 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off >= W; off >>= 1) v += shfl_xor_t(v, off);
        if (lane < W) red[wv][lane][k] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < W) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            double t = 0.0;
            for (int w = 0; w < BLOCK / 64; ++w) t += red[w][threadIdx.x][k];
            partials[((size_t)blockIdx.x * Bp + blockIdx.y * W + threadIdx.x) * NA + k] = t;
        }
    }
}

// Primal half (step.py:25-30 / :78-82): x+ = clamp(x - tau (c - K'y), l, u), xbar = x+ + (x+ - x), x_prev = x;
// fixed step: x_sum += eta x+ (pdhg.py:107); adaptive: x_sum += wpend x (the previous iteration's term, its weight is known now)
template <typename T, bool ADAPT> struct BPrimal {
    static constexpr int NA = 0;
    T* X; T* Xprev; T* Xbar; T* Xsum; const T* c; const T* l; const T* u; int cs, ls, us;
    const T* eta; const T* omega; const T* wpend;
    __device__ void operator()(int j, size_t at, int b, int, T kty, double*) const
    {
        const T xo = X[at];
        if (ADAPT) Xsum[at] = Xsum[at] + wpend[b] * xo;
        const T tau = eta[b] / omega[b];
        const T v = primal_step(xo, tau, BCOL(c, cs, j, at), kty, BCOL(l, ls, j, at), BCOL(u, us, j, at));
        X[at] = v;
        Xprev[at] = xo;
        Xbar[at] = v + (v - xo);                       // theta = 1 (pdhg.py:27)
        if (!ADAPT) Xsum[at] = Xsum[at] + eta[b] * v;
    }
};

// Dual half (step.py:33-38 / :85-90): y+ = y + sigma (q - K xbar), first m_ineq rows >= 0, y_prev = y; adaptive: dy = y+ - y
// kept for K'dy and ||dy||^2 partials (step.py:92-100)
template <typename T, bool ADAPT> struct BDual {
    static constexpr int NA = ADAPT ? 1 : 0;
    T* Y; T* Yprev; T* Ysum; T* DY; const T* q; int qs; const T* eta; const T* omega; const T* wpend; int ineq_end;
    __device__ void operator()(int i, size_t at, int b, int, T kx, double* acc) const
    {
        const T yo = Y[at];
        if (ADAPT) Ysum[at] = Ysum[at] + wpend[b] * yo;
        const T sigma = eta[b] * omega[b];
        const T v = dual_step(i, ineq_end, yo, sigma, BCOL(q, qs, i, at), kx);
        Y[at] = v;
        Yprev[at] = yo;
        if (!ADAPT) {
            Ysum[at] = Ysum[at] + eta[b] * v;
        } else {
            const T d = v - yo;
            DY[at] = d;
            acc[0] += (double)d * (double)d;
        }
    }
};

// Reflected Halpern iteration per column (pdlp_batch_halpern_iterate; the reference has no counterpart).  The weights of column
// b at iteration t = t_since[b] + it since its last restart: a = (t+1)/(t+2), bw = 1/(t+2), divided in double and rounded once
// to the working type (rules.halpern_weights); t stays in 64 bits.
template <typename T> struct BHalpernWeights {
    const int64_t* t_since; int64_t it;
    __device__ void operator()(int b, T& a, T& bw) const
    {
        const int64_t t = t_since[b] + it;
        const double t2 = (double)(t + 2);
        a = (T)((double)(t + 1) / t2);
        bw = (T)(1.0 / t2);
    }
};

// Primal half: the candidate x' = BPrimal<T, false>'s X goes to x_avg and xbar = x' + (x' - x) is stored as there (one fixed
// batched PDHG step from z bit for bit); the iterate becomes the reflected point pulled towards the anchor, x+ = a xbar + bw x_last
// (HalpernPrimalEpi).  In place: the launch gathers y and touches element `at` of the x side only.  No sums, no x_prev.
template <typename T> struct BHalpernPrimal {
    static constexpr int NA = 0;
    T* X; T* Xbar; T* Xcand; const T* Xlast; const T* c; const T* l; const T* u; int cs, ls, us;
    const T* eta; const T* omega; BHalpernWeights<T> w;
    __device__ void operator()(int j, size_t at, int b, int, T kty, double*) const
    {
        T a, bw;
        w(b, a, bw);                                  // before the first store: the load of t_since and the divisions overlap the others
        const T xo = X[at], xl = Xlast[at];
        const T tau = eta[b] / omega[b];
        const T v = primal_step(xo, tau, BCOL(c, cs, j, at), kty, BCOL(l, ls, j, at), BCOL(u, us, j, at));
        Xcand[at] = v;
        const T xb = v + (v - xo);
        Xbar[at] = xb;
        X[at] = a * xb + bw * xl;
    }
};

// Dual half: the candidate y' = BDual<T, false>'s Y goes to y_avg; y+ = a (2y' - y) + bw y_last (HalpernDualEpi).  In place: the
// launch gathers xbar and touches element `at` of the y side only.
template <typename T> struct BHalpernDual {
    static constexpr int NA = 0;
    T* Y; T* Ycand; const T* Ylast; const T* q; int qs; const T* eta; const T* omega; int ineq_end; BHalpernWeights<T> w;
    __device__ void operator()(int i, size_t at, int b, int, T kx, double*) const
    {
        T a, bw;
        w(b, a, bw);                                  // (as in the primal half)
        const T yo = Y[at], yl = Ylast[at];
        const T sigma = eta[b] * omega[b];
        const T v = dual_step(i, ineq_end, yo, sigma, BCOL(q, qs, i, at), kx);
        Ycand[at] = v;
        Y[at] = a * ((T)2 * v - yo) + bw * yl;
    }
};

// the adaptive rule's other two sums (step.py:96-100): (K'dy).dx and ||dx||^2; rows of K', gathers dy
template <typename T> struct BDen {
    static constexpr int NA = 2;
    const T* X; const T* Xprev;
    __device__ void operator()(int j, size_t at, int, int, T kdy, double* acc) const
    {
        const T dx = X[at] - Xprev[at];
        acc[0] += (double)kdy * (double)dx;
        acc[1] += (double)dx * (double)dx;
    }
};

// KKT, variable side (helpers.py:21-37,75-82,93-95): ||c - K'y - lam||^2, l_dual'max(lam,0), u_dual'min(lam,0), c'x -- the
// arithmetic of KktDualEpi per column.  box(): g = c - K'y of row j and lam = project_lambda_box(g) (helpers.py:3-39) with the
// bounds as the dual objective takes them (an infinite one counts 0), un-scaled on request -- the sums and the report's store
template <typename T> struct BBox { T g, lam, ld, ud; };
template <typename T, bool UNSCALE> struct BKktDual {
    static constexpr int NA = 4;
    const T* X; const T* c; const T* l; const T* u; int cs, ls, us; const T* dcol; int dper;
    __device__ BBox<T> box(int j, size_t at, T kty) const
    {
        T lo = BCOL(l, ls, j, at), hi = BCOL(u, us, j, at);
        T g = BCOL(c, cs, j, at) - kty;
        if (UNSCALE) {            // K_u'(D_row y) = (K_s'y)/D_col, l_u = l_s D_col
            const T d = BCOL(dcol, dper, j, at);
            g = g / d; lo = lo * d; hi = hi * d;
        }
        const BoxLam<T> b = project_lambda(g, lo, hi);
        return {g, b.lam, b.ninf ? (T)0 : lo, b.pinf ? (T)0 : hi};
    }
    __device__ void operator()(int j, size_t at, int, int, T kty, double* acc) const
    {
        const BBox<T> v = box(j, at, kty);
        T cj = BCOL(c, cs, j, at), xj = X[at];
        if (UNSCALE) {            // c_u = c_s/D_col, x_u = D_col x
            const T d = BCOL(dcol, dper, j, at);
            cj = cj / d; xj = xj * d;
        }
        const T r = v.g - v.lam;
        acc[0] += (double)r * (double)r;
        acc[1] += (double)v.ld * (double)(v.lam > (T)0 ? v.lam : (T)0);
        acc[2] += (double)v.ud * (double)(v.lam < (T)0 ? v.lam : (T)0);
        acc[3] += (double)cj * (double)xj;
    }
};

// KKT, constraint side (helpers.py:77,87-91): ||(K x - q) with inequality rows clipped at 0||^2, q'y
template <typename T, bool UNSCALE> struct BKktPrimal {
    static constexpr int NA = 2;
    const T* Y; const T* q; int qs; const T* drow; int dper; int ineq_end;
    __device__ void operator()(int i, size_t at, int, int, T kx, double* acc) const
    {
        T qi = BCOL(q, qs, i, at), yi = Y[at];
        T r = kx - qi;
        if (UNSCALE) {            // K_u (D_col x) = (K_s x)/D_row, q_u = q_s/D_row, y_u = D_row y
            const T d = BCOL(drow, dper, i, at);
            r = r / d; qi = qi / d; yi = yi * d;
        }
        if (i < ineq_end && r > (T)0) r = (T)0;
        acc[0] += (double)r * (double)r;
        acc[1] += (double)qi * (double)yi;
    }
};

// Solution report per column (pdlp_batch_report, pdlp_batch_retire): the KKT sums of BKktDual / BKktPrimal with the iterate of
// the side, the reduced cost lam resp. the row activity K x stored beside them at [row][id] of the caller's [len][N] arrays (null:
// not stored) -- UNSCALE: lam_u = lam_s / D_col, act_u = (K_s x_s) / D_row.  The report is N = Bp, id = b, no iterate.
template <typename T, bool UNSCALE> struct BReportDual {
    static constexpr int NA = 4;
    BKktDual<T, UNSCALE> kkt; T* Xout; T* RC; int N;
    __device__ void operator()(int j, size_t at, int b, int id, T kty, double* acc) const
    {
        const size_t to = (size_t)j * N + id;
        if (Xout) Xout[to] = kkt.X[at];
        if (RC) RC[to] = kkt.box(j, at, kty).lam;
        kkt(j, at, b, id, kty, acc);
    }
};
template <typename T, bool UNSCALE> struct BReportPrimal {
    static constexpr int NA = 2;
    BKktPrimal<T, UNSCALE> kkt; T* Yout; T* ACT; int N;
    __device__ void operator()(int i, size_t at, int b, int id, T kx, double* acc) const
    {
        const size_t to = (size_t)i * N + id;
        if (Yout) Yout[to] = kkt.Y[at];
        if (ACT) ACT[to] = UNSCALE ? kx / BCOL(kkt.drow, kkt.dper, i, at) : kx;
        kkt(i, at, b, id, kx, acc);
    }
};

// the plain population product (pdlp_batch_product): Vout[row][b] = the row sum, no state
template <typename T> struct BStore {
    static constexpr int NA = 0;
    T* Vout;
    __device__ void operator()(int, size_t at, int, int, T s, double*) const { Vout[at] = s; }
};

// Which columns a launch serves.  pick(b, W, id) for the lane's column b: id >= 0 when b takes part -- the column of the
// destination under which an epilogue files its stores (b itself unless listed) --, else -1; false when no column of b's group
// takes part and the workgroup leaves at once (uniform over the workgroup).
struct BSelLive {               // the live columns (every iteration, the KKT passes)
    const int32_t* live;
    __device__ bool pick(int b, int, int& id) const { id = live[b] ? b : -1; return true; }
};
struct BSelAll {                // every LP of the batch, b < B, frozen or not (the report is wanted when all are frozen; the plain
    int B;                      // product); padding columns are neither read nor written
    __device__ bool pick(int b, int, int& id) const { id = b < B ? b : -1; return true; }
};
struct BSelList {               // column cols[i] of the batch under column ids[i] of [len][N] arrays (retirement); an entry with a
    int count; const int32_t* cols; const int32_t* ids; int Bp, N;       // column outside [0, Bp) or an id outside [0, N) is skipped
    __device__ bool pick(int b, int W, int& id) const
    {
        bool any = false;
        id = -1;
        for (int i = 0; i < count; ++i) {
            const int c = cols[i], v = ids[i];
            if (c < 0 || c >= Bp || v < 0 || v >= N) continue;
            any = any || c / W == (int)blockIdx.y;
            if (c == b) id = v;
        }
        return any;             // a group without a listed column: its partials are never read (k_batch_finalize sums the listed)
    }
};

// the row walk of a launch for column b of its group: the matrix (rows x cols, CSR) times column b of Vin[cols][Bp], the epilogue
// per row.  PERLP: va is the population of values [nnz][Bp] and item p of this column is va[p * Bp + b]; else va[p] serves all
template <typename T, int W, bool PERLP, class Epi>
__device__ __forceinline__ void batch_rows(int rows, const int64_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                           const T* __restrict__ va, const T* __restrict__ Vin, int Bp, int b, int id, const Epi& epi,
                                           double* acc)
{
    constexpr int RPW = 64 / W;
    const int sub = (threadIdx.x & 63) / W;
    const int wave = (blockIdx.x * BLOCK + threadIdx.x) >> 6, nwaves = gridDim.x * (BLOCK / 64);
    for (int r0 = wave * RPW; r0 < rows; r0 += nwaves * RPW) {
        const int r = r0 + sub;
        if (r < rows) {
            T s = (T)0;
            const int64_t e = rp[r + 1];
            if (PERLP) {
                for (int64_t p = rp[r]; p < e; ++p) s += va[(size_t)p * Bp + b] * Vin[(size_t)ci[p] * Bp + b];
            } else {
                for (int64_t p = rp[r]; p < e; ++p) s += va[p] * Vin[(size_t)ci[p] * Bp + b];
            }
            epi(r, (size_t)r * Bp + b, b, id, s, acc);
        }
    }
}

// one product of the matrix (rows x cols, CSR) with a population Vin[cols][Bp], the epilogue per (row, column the selector picks)
template <typename T, int W, bool PERLP, class Sel, class Epi>
__global__ __launch_bounds__(BLOCK) void k_batch_mv(int rows, const int64_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                                    const T* __restrict__ va, const T* __restrict__ Vin, int Bp, Sel sel, Epi epi,
                                                    double* __restrict__ partials)
{
    const int b = blockIdx.y * W + (threadIdx.x & 63) % W;
    int id;
    if (!sel.pick(b, W, id)) return;
    double acc[Epi::NA > 0 ? Epi::NA : 1] = {0.0};
    if (id >= 0) batch_rows<T, W, PERLP>(rows, rp, ci, va, Vin, Bp, b, id, epi, acc);
    if (Epi::NA > 0) batch_store_partials<W, Epi::NA>(acc, partials, Bp);
}

// sum over g < nblocks of partials[(g * Bp + b) * na + a] by one workgroup, in a fixed order: thread t adds g = t, t + 256, ...
// in turn, then the lanes of a wave (xor tree) and the four waves in order.  Valid in thread 0.
__device__ __forceinline__ double batch_block_sum(const double* __restrict__ partials, int nblocks, int Bp, int na, int b, int a)
{
    __shared__ double wsum[BLOCK / 64];
    double s = 0.0;
    for (int g = threadIdx.x; g < nblocks; g += BLOCK) s += partials[((size_t)g * Bp + b) * na + a];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += shfl_xor_t(s, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < BLOCK / 64; ++w) t += wsum[w];
    return t;
}

// out[b * stride + off + a] = sum over blocks of partials[block][b][a], a < na: one workgroup per (i, a); b = i, or with a list
// b = cols[i] (an entry that BSelList skips is skipped here)
__global__ __launch_bounds__(BLOCK) void k_batch_finalize(const double* __restrict__ partials, int nblocks, int Bp, int na,
                                                          const int32_t* __restrict__ cols, const int32_t* __restrict__ ids, int N,
                                                          double* __restrict__ out, int stride, int off)
{
    const int i = blockIdx.x / na, a = blockIdx.x - i * na;
    const int b = cols ? cols[i] : i;
    if (cols && (b < 0 || b >= Bp || ids[i] < 0 || ids[i] >= N)) return;      // (uniform over the workgroup)
    const double s = batch_block_sum(partials, nblocks, Bp, na, b, a);
    if (threadIdx.x == 0) out[(size_t)b * stride + off + a] = s;
}

// adaptive_one_step_pdhg's step-size rule per LP (step.py:92-115, one trial: quirk Q1), then the bookkeeping of pdhg.py:107-112:
// the step just taken gets weight eta_w (added to the sums by the next iteration, wpend), eta_sum += eta_w, eta = eta'.
// One workgroup per LP: it reduces the LP's three partial sums, thread 0 applies the rule.  k_global + 1 is the iteration count
// of the batch after this step; an LP admitted later (k_start[b] > 0, pdlp_batch_iterate_from) counts from its admission.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_batch_adapt(int Bp, const int32_t* __restrict__ live, const double* __restrict__ part_dy,
                                                       int gm, const double* __restrict__ part_den, int gn, T* eta,
                                                       const T* __restrict__ omega, T* eta_sum, T* wpend, int64_t k_global,
                                                       const int64_t* __restrict__ k_start)
{
    const int b = blockIdx.x;
    if (!live[b]) return;                       // (uniform over the workgroup)
    const int64_t k = k_start ? k_global - k_start[b] : k_global;      // the LP's own count: it entered its column at k_start[b]
    const double dyy = batch_block_sum(part_dy, gm, Bp, 1, b, 0);
    const double dkd = batch_block_sum(part_den, gn, Bp, 2, b, 0);
    const double dxx = batch_block_sum(part_den, gn, Bp, 2, b, 1);
    if (threadIdx.x != 0) return;
    const T e = eta[b], om = omega[b];
    const T den = (T)2 * (T)dkd;                                          // step.py:96
    T eta_bar, t1;
    if (den != (T)0) {                                                    // step.py:99-102
        const T nx = (T)sqrt(dxx), ny = (T)sqrt(dyy);
        const T num = om * (nx * nx) + (ny * ny) / om;
        eta_bar = num / (T)fabs((double)den);
        t1 = (T)(1.0 - pow((double)(k + 1), -0.3)) * eta_bar;
    } else {                                                              // step.py:104-105
        eta_bar = (T)INFINITY;
        t1 = (T)INFINITY;
    }
    const T t2 = (T)(1.0 + pow((double)(k + 1), -0.6)) * e;              // step.py:107
    const T ep = t1 < t2 ? t1 : t2;                                       // step.py:108
    const T ew = e <= eta_bar ? e : ep;                                   // step.py:110-115
    eta_sum[b] = eta_sum[b] + ew;
    wpend[b] = ew;
    eta[b] = ep;
}

// fixed step: eta_sum += eta, `iters` times (pdhg.py:109; eta does not change)
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_batch_etasum(int Bp, const int32_t* __restrict__ live, const T* __restrict__ eta, T* eta_sum, int iters)
{
    for (int b = blockIdx.x * BLOCK + threadIdx.x; b < Bp; b += gridDim.x * BLOCK) {
        if (!live[b]) continue;
        T s = eta_sum[b];
        const T e = eta[b];
        for (int i = 0; i < iters; ++i) s = s + e;
        eta_sum[b] = s;
    }
}

// averaged iterate (pdhg.py:118-119): [adaptive: the current iterate's pending term first] V_avg = V_sum / eta_sum
template <typename T, bool ADAPT>
__global__ __launch_bounds__(BLOCK) void k_batch_average(int64_t total, int Bp, const int32_t* __restrict__ live, T* Vsum,
                                                         const T* __restrict__ V, T* __restrict__ Vavg, const T* __restrict__ wpend,
                                                         const T* __restrict__ eta_sum)
{
    for (int64_t at = (int64_t)blockIdx.x * BLOCK + threadIdx.x; at < total; at += (int64_t)gridDim.x * BLOCK) {
        const int b = (int)(at % Bp);
        if (!live[b]) continue;
        T s = Vsum[at];
        if (ADAPT) {
            s = s + wpend[b] * V[at];
            Vsum[at] = s;
        }
        Vavg[at] = s / eta_sum[b];
    }
}

__global__ void k_batch_zero_pending(int Bp, const int32_t* __restrict__ live, void* wpend, int es)
{
    for (int b = blockIdx.x * BLOCK + threadIdx.x; b < Bp; b += gridDim.x * BLOCK)
        if (live[b]) {
            if (es == 4) ((float*)wpend)[b] = 0.0f;
            else ((double*)wpend)[b] = 0.0;
        }
}

// restarts per LP (pdhg.py:131-146,150-151,58-64): act 0 keep, 1 restart at the current iterate, 2 at the average (which becomes
// current).  A restarted column: sums zeroed, partial of ||v - v_last||^2 (enhancements.py:74-75), v_last = v (mark).  With
// eta_sum / wpend given (the x launch), the LP's eta_sum and pending weight are zeroed as well.
template <typename T, int W>
__global__ __launch_bounds__(BLOCK) void k_batch_restart(int rows, int Bp, const int32_t* __restrict__ act, T* V,
                                                         const T* __restrict__ Vavg, T* Vsum, T* Vlast, T* eta_sum, T* wpend,
                                                         double* __restrict__ partials)
{
    constexpr int RPW = 64 / W;
    const int lane = threadIdx.x & 63, sub = lane / W;
    const int b = blockIdx.y * W + lane % W;
    const int wave = (blockIdx.x * BLOCK + threadIdx.x) >> 6, nwaves = gridDim.x * (BLOCK / 64);
    const int a = act[b];
    double acc[1] = {0.0};
    if (a != 0) {
        for (int r = wave * RPW + sub; r < rows; r += nwaves * RPW) {
            const size_t at = (size_t)r * Bp + b;
            const T v = a == 2 ? Vavg[at] : V[at];
            if (a == 2) V[at] = v;
            Vsum[at] = (T)0;
            const T d = v - Vlast[at];
            acc[0] += (double)d * (double)d;
            Vlast[at] = v;
        }
        if (eta_sum && wave == 0 && sub == 0) {
            eta_sum[b] = (T)0;
            wpend[b] = (T)0;
        }
    }
    batch_store_partials<W, 1>(acc, partials, Bp);
}
// ---- streaming a family through the columns (pdlp_batch_admit, pdlp_batch_retire) ----------------------------------------------
// Both take a list: column cols[i] of the batch and column ids[i] of a [len][N] array of the caller (the feed, the results).
// An entry with a column outside [0, Bp) or an id outside [0, N) is skipped.  Retirement is the report (BReportDual / BReportPrimal)
// under BSelList.

// admission, one side (the n rows, the m rows or the nnz items): element (row, i), i fastest, so columns listed next to each other
// are stored next to each other.  d0..d2 <- s0..s2: the per-LP vectors (or value populations) of this side, null = none;
// V = Vlast = V0 (null: zeros), Vsum = 0 when the side has an iterate; with eta given (the n rows) the LP's scalars as well.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_batch_admit(int64_t rows, int count, const int32_t* __restrict__ cols,
                                                       const int32_t* __restrict__ ids, int Bp, int N, T* d0, const T* __restrict__ s0,
                                                       T* d1, const T* __restrict__ s1, T* d2, const T* __restrict__ s2, T* V, T* Vlast,
                                                       T* Vsum, const T* __restrict__ V0, T* eta, T* omega, T* eta_sum, T* wpend,
                                                       const T* __restrict__ feta, const T* __restrict__ fomega)
{
    const int64_t total = rows * count;
    for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * BLOCK) {
        const int64_t r = e / count;
        const int i = (int)(e - r * count);
        const int col = cols[i], id = ids[i];
        if (col < 0 || col >= Bp || id < 0 || id >= N) continue;
        const size_t at = (size_t)r * Bp + col, from = (size_t)r * N + id;
        if (d0) d0[at] = s0[from];
        if (d1) d1[at] = s1[from];
        if (d2) d2[at] = s2[from];
        if (V) {
            const T v = V0 ? V0[from] : (T)0;
            V[at] = v;
            Vlast[at] = v;
            Vsum[at] = (T)0;
        }
        if (eta && r == 0) {
            eta[col] = feta[id];
            omega[col] = fomega[id];
            eta_sum[col] = (T)0;
            wpend[col] = (T)0;
        }
    }
}
#undef BCOL
