// pdlp_kernel_mv.inc -- multi-vector kernels: a population of up to 32 points advanced together (fishnet warm start).
// Part of pdlp_hip.hip (included inside its anonymous namespace; not a translation unit of its own).
//
// The reference's fishnet (PDLP/spectral_casting.py:65-159) runs fixed-step PDHG on an n x j matrix of points
// (PDHG_step :254-293) and ranks them by duality gap (get_best_pts :191-252).  Here the population is stored
// row-major, V[row][NVP]: an item (row r, column c, value v) of the matrix contributes v * V[c][0..NVP) to NVP
// row sums at once -- ONE fully coalesced line per item instead of NVP scattered gathers, and the matrix is read once
// per NVP points.  NVP lanes work on an item (lane % NVP = the point), a wave advances 64/NVP rows at a time, each
// lane group walking its row's items in CSR order (no LDS; rows of LP matrices are short).
// ------------------------------------------------------------------------------------------------
template <typename T> struct PrimalMV {          // PDHG_step :277-284: x+ = clamp(x - tau (c - K'y), l, u), xbar
    static constexpr int NA = 0;
    const T* X; T* Xnew; T* Xbar; const T* c; const T* l; const T* u; T tau, theta;
    __device__ void operator()(int j, size_t at, T kty, double*) const
    {
        const T xo = X[at];
        const T v = primal_step(xo, tau, c[j], kty, l[j], u[j]);
        Xnew[at] = v;
        Xbar[at] = v + theta * (v - xo);
    }
};

template <typename T> struct DualMV {            // PDHG_step :287-292: y+ = y + sigma (q - K xbar), first m_ineq rows >= 0
    static constexpr int NA = 0;
    const T* Y; T* Ynew; const T* q; T sigma; int ineq_end;
    __device__ void operator()(int i, size_t at, T kxbar, double*) const
    {
        const T v = dual_step(i, ineq_end, Y[at], sigma, q[i], kxbar);
        Ynew[at] = v;
    }
};

template <typename T> struct StoreMV {           // fishnet :100: pts_y = K @ pts
    static constexpr int NA = 0;
    T* Out;
    __device__ void operator()(int, size_t at, T kx, double*) const { Out[at] = kx; }
};

template <typename T> struct GapMV {             // get_best_pts :222-233: c'x, l_dual'max(lam,0), u_dual'min(lam,0) per point
    static constexpr int NA = 3;
    const T* X; const T* c; const T* l; const T* u;
    __device__ void operator()(int j, size_t at, T kty, double* acc) const
    {
        const T cj = c[j], lo = l[j], hi = u[j];
        const BoxLam<T> b = project_lambda(cj - kty, lo, hi);
        const T lam = b.lam;
        acc[0] += (double)cj * (double)X[at];
        acc[1] += (double)(b.ninf ? (T)0 : lo) * (double)(lam > (T)0 ? lam : (T)0);
        acc[2] += (double)(b.pinf ? (T)0 : hi) * (double)(lam < (T)0 ? lam : (T)0);
    }
};

// partial sums of NA quantities per point: lanes of equal point over the wave, then the four waves; partials[block][point][NA]
template <int NVP, int NA> __device__ __forceinline__ void mv_store_partials(double* acc, double* partials)
{
    __shared__ double red[BLOCK / 64][NVP][NA > 0 ? NA : 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off >= NVP; off >>= 1) v += shfl_xor_t(v, off);
        if (lane < NVP) red[wv][lane][k] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < NVP) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            double t = 0.0;
            for (int w = 0; w < BLOCK / 64; ++w) t += red[w][threadIdx.x][k];
            partials[((size_t)blockIdx.x * NVP + threadIdx.x) * NA + k] = t;
        }
    }
}

template <typename T, int NVP, class Epi>
__global__ __launch_bounds__(BLOCK) void k_csr_mv(int rows, const int64_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                                  const T* __restrict__ va, const T* __restrict__ Vin, Epi epi,
                                                  double* __restrict__ partials)
{
    constexpr int RPW = 64 / NVP;                        // rows a wave works on at a time
    const int lane = threadIdx.x & 63, vec = lane % NVP, sub = lane / NVP;
    const int wave = (blockIdx.x * BLOCK + threadIdx.x) >> 6, nwaves = gridDim.x * (BLOCK / 64);
    double acc[Epi::NA > 0 ? Epi::NA : 1] = {0.0};
    for (int r0 = wave * RPW; r0 < rows; r0 += nwaves * RPW) {
        const int r = r0 + sub;
        if (r < rows) {
            T s = (T)0;
            const int64_t e = rp[r + 1];
            for (int64_t p = rp[r]; p < e; ++p) s += va[p] * Vin[(size_t)ci[p] * NVP + vec];
            epi(r, (size_t)r * NVP + vec, s, acc);
        }
    }
    if (Epi::NA > 0) mv_store_partials<NVP, Epi::NA>(acc, partials);
}

// q'y per point (get_best_pts :224): partials[block][point][1]
template <typename T, int NVP>
__global__ __launch_bounds__(BLOCK) void k_mv_dot(int len, const T* __restrict__ w, const T* __restrict__ V, double* __restrict__ partials)
{
    constexpr int RPW = 64 / NVP;
    const int lane = threadIdx.x & 63, vec = lane % NVP, sub = lane / NVP;
    const int wave = (blockIdx.x * BLOCK + threadIdx.x) >> 6, nwaves = gridDim.x * (BLOCK / 64);
    double acc[1] = {0.0};
    for (int r = wave * RPW + sub; r < len; r += nwaves * RPW) acc[0] += (double)w[r] * (double)V[(size_t)r * NVP + vec];
    mv_store_partials<NVP, 1>(acc, partials);
}

// out[e] = sum over blocks of partials[block][e], e < width, fixed order
__global__ __launch_bounds__(BLOCK) void k_mv_finalize(const double* __restrict__ partials, int nblocks, int width, double* __restrict__ out)
{
    for (int e = threadIdx.x; e < width; e += BLOCK) {
        double s = 0.0;
        for (int b = 0; b < nblocks; ++b) s += partials[(size_t)b * width + e];
        out[e] = s;
    }
}

// OUT[r][t] = sum_p V[r][p] W[p][t]  (fishnet breeding, spectral_casting.py:133-141: columns of W are convex weights); p in order
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_mv_combine(int64_t rows, int j, const T* __restrict__ V, const T* __restrict__ W, int nw,
                                                      T* __restrict__ Out)
{
    __shared__ T w[32 * 32];
    for (int e = threadIdx.x; e < j * nw; e += BLOCK) w[e] = W[e];
    __syncthreads();
    const int64_t total = rows * nw;
    for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * BLOCK) {
        const int64_t r = e / nw;
        const int t = (int)(e - r * nw);
        T s = (T)0;
        for (int p = 0; p < j; ++p) s += V[r * j + p] * w[p * nw + t];
        Out[e] = s;
    }
}
