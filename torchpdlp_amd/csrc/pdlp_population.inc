// pdlp_population.inc -- launchers of the population kernels (pdlp_kernel_mv.inc: 8, 16 or 32 vectors per product): fixed-step
// PDHG steps, duality gaps and the plain product over a population, each dispatched on the vector count; and pdlp_mv_combine.
// Part of pdlp_hip.hip (included at file scope; not a translation unit of its own).  Needs: pdlp_handle.inc.
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int MV_GAP_GRID = 256;
inline int mv_grid(int64_t rows, int nvp)
{
    const int64_t per_block = (int64_t)(64 / nvp) * (BLOCK / 64);
    const int64_t g = (rows + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

template <typename T, int NVP> int mv_steps_n(pdlp_handle h, int steps, double eta, double omega, double theta, T* X, T* Y, T* work)
{
    const int64_t n = h->p.n, m = h->p.m;
    const T e = (T)eta, w = (T)omega;
    const T tau = (T)(e / w), sigma = (T)(e * w);                 // (rounded like k_set_step)
    T *Xa = X, *Xb = work, *Xbar = work + n * NVP, *Ya = Y, *Yb = work + 2 * n * NVP;
    for (int s = 0; s < steps; ++s) {
        PrimalMV<T> ep{Xa, Xb, Xbar, (const T*)h->p.c, (const T*)h->p.l, (const T*)h->p.u, tau, (T)theta};
        hipLaunchKernelGGL((k_csr_mv<T, NVP, PrimalMV<T>>), dim3(mv_grid(n, NVP)), dim3(BLOCK), 0, h->stream, (int)n, h->p.KT_rowptr,
                           h->p.KT_colidx, (const T*)h->p.KT_val, (const T*)Ya, ep, (double*)nullptr);
        DualMV<T> ed{Ya, Yb, (const T*)h->p.q, sigma, h->ineq_end};
        hipLaunchKernelGGL((k_csr_mv<T, NVP, DualMV<T>>), dim3(mv_grid(m, NVP)), dim3(BLOCK), 0, h->stream, (int)m, h->p.K_rowptr,
                           h->p.K_colidx, (const T*)h->p.K_val, (const T*)Xbar, ed, (double*)nullptr);
        T* t = Xa; Xa = Xb; Xb = t;
        t = Ya; Ya = Yb; Yb = t;
    }
    HIP_TRY(hipGetLastError());
    if (steps & 1) {
        HIP_TRY(hipMemcpyAsync(X, Xa, (size_t)n * NVP * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(Y, Ya, (size_t)m * NVP * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
    }
    return PDLP_OK;
}

template <typename T, int NVP> int mv_gap_n(pdlp_handle h, const T* X, const T* Y, double* work, double* gaps)
{
    const int64_t n = h->p.n, m = h->p.m;
    const int ga = mv_grid(n, NVP) < MV_GAP_GRID ? mv_grid(n, NVP) : MV_GAP_GRID, gb = mv_grid(m, NVP) < MV_GAP_GRID ? mv_grid(m, NVP) : MV_GAP_GRID;
    double* pa = work;                                   // [ga][NVP][3]
    double* pb = work + (size_t)MV_GAP_GRID * NVP * 3;   // [gb][NVP][1]
    double* out = pb + (size_t)MV_GAP_GRID * NVP;        // [NVP][3] then [NVP]
    GapMV<T> eg{X, (const T*)h->p.c, (const T*)h->p.l, (const T*)h->p.u};
    hipLaunchKernelGGL((k_csr_mv<T, NVP, GapMV<T>>), dim3(ga), dim3(BLOCK), 0, h->stream, (int)n, h->p.KT_rowptr, h->p.KT_colidx,
                       (const T*)h->p.KT_val, Y, eg, pa);
    hipLaunchKernelGGL((k_mv_dot<T, NVP>), dim3(gb), dim3(BLOCK), 0, h->stream, (int)m, (const T*)h->p.q, Y, pb);
    hipLaunchKernelGGL(k_mv_finalize, dim3(1), dim3(BLOCK), 0, h->stream, pa, ga, NVP * 3, out);
    hipLaunchKernelGGL(k_mv_finalize, dim3(1), dim3(BLOCK), 0, h->stream, pb, gb, NVP, out + NVP * 3);
    HIP_TRY(hipGetLastError());
    double r[32 * 4];
    HIP_TRY(hipMemcpyAsync(r, out, (size_t)NVP * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int v = 0; v < NVP; ++v) {                      // get_best_pts :231-233 in the working precision
        const T p = (T)r[3 * v], lp = (T)r[3 * v + 1], un = (T)r[3 * v + 2], d = (T)r[NVP * 3 + v];
        const T adj = d + lp + un;
        gaps[v] = (double)(T)(adj - p);
    }
    return PDLP_OK;
}

template <typename T, int NVP> int mv_product_n(pdlp_handle h, const T* X, T* Y)
{
    const int64_t m = h->p.m;
    StoreMV<T> st{Y};
    hipLaunchKernelGGL((k_csr_mv<T, NVP, StoreMV<T>>), dim3(mv_grid(m, NVP)), dim3(BLOCK), 0, h->stream, (int)m, h->p.K_rowptr,
                       h->p.K_colidx, (const T*)h->p.K_val, X, st, (double*)nullptr);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

template <typename T> int mv_product_t(pdlp_handle h, int nvp, const void* X, void* Y)
{
    if (nvp == 8) return mv_product_n<T, 8>(h, (const T*)X, (T*)Y);
    if (nvp == 16) return mv_product_n<T, 16>(h, (const T*)X, (T*)Y);
    return mv_product_n<T, 32>(h, (const T*)X, (T*)Y);
}

template <typename T> int mv_steps_t(pdlp_handle h, int nvp, int steps, double eta, double omega, double theta, void* X, void* Y, void* work)
{
    if (nvp == 8) return mv_steps_n<T, 8>(h, steps, eta, omega, theta, (T*)X, (T*)Y, (T*)work);
    if (nvp == 16) return mv_steps_n<T, 16>(h, steps, eta, omega, theta, (T*)X, (T*)Y, (T*)work);
    return mv_steps_n<T, 32>(h, steps, eta, omega, theta, (T*)X, (T*)Y, (T*)work);
}

template <typename T> int mv_gap_t(pdlp_handle h, int nvp, const void* X, const void* Y, void* work, double* gaps)
{
    if (nvp == 8) return mv_gap_n<T, 8>(h, (const T*)X, (const T*)Y, (double*)work, gaps);
    if (nvp == 16) return mv_gap_n<T, 16>(h, (const T*)X, (const T*)Y, (double*)work, gaps);
    return mv_gap_n<T, 32>(h, (const T*)X, (const T*)Y, (double*)work, gaps);
}

}  // namespace

extern "C" {

int pdlp_mv_combine(int dtype, int64_t rows, int j, const void* V, const void* W, int nw, void* OUT, void* stream)
{
    if (rows < 0 || j < 1 || j > 32 || nw < 1 || nw > 32 || !V || !W || !OUT || (dtype != PDLP_F32 && dtype != PDLP_F64)) return PDLP_ERR_INVALID;
    if (rows == 0) return PDLP_OK;
    hipStream_t s = (hipStream_t)stream;
    WITH_T(dtype, hipLaunchKernelGGL(k_mv_combine<T>, dim3(grid_for(rows * nw)), dim3(BLOCK), 0, s, rows, j, (const T*)V, (const T*)W, nw, (T*)OUT));
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

}  // extern "C"
