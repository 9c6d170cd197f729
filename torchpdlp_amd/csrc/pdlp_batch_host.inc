// pdlp_batch_host.inc -- host side of the batched solves (pdlp_batch_*, include/pdlp_hip.h): launch shapes and the C entry points.
// Part of pdlp_hip.hip (included at file scope after the other entry points; not a translation unit of its own).
// Kernels: pdlp_kernel_batch.inc.  Instantiated per (dtype, W, shared or per-LP matrix values, epilogue); every other flag (shared
// or per-LP vectors, the iteration count) is a launch argument.  With matrices attached (pdlp_batch_attach_matrices) every product
// here reads the per-LP values and the un-scaling epilogues the per-LP Ruiz factors.
// ------------------------------------------------------------------------------------------------
namespace {

int batch_check(pdlp_handle h, const pdlp_batch* b)
{
    if (!h || !b) return PDLP_ERR_INVALID;
    if (b->W != 8 && b->W != 16 && b->W != 32) return PDLP_ERR_INVALID;
    if (b->B < 1 || b->Bp < b->B || b->Bp % b->W != 0) return PDLP_ERR_INVALID;
    if (!b->c || !b->q || !b->l || !b->u || !b->x || !b->x_prev || !b->xbar || !b->x_sum || !b->x_avg || !b->x_last || !b->y ||
        !b->y_prev || !b->y_sum || !b->y_avg || !b->y_last || !b->dy || !b->eta || !b->omega || !b->eta_sum || !b->wpend ||
        !b->live || !b->action || !b->part || !b->out)
        return PDLP_ERR_INVALID;
    if (h->nl != h->p.n || h->ml != h->p.m || h->mixed || h->delta) return PDLP_ERR_STATE;     // single GPU, one precision
    if (h->p.n < 1 || h->p.m < 1) return PDLP_ERR_INVALID;
    if (h->bm.K_val && h->bm.Bp != b->Bp) return PDLP_ERR_INVALID;      // the attached populations have another width
    return PDLP_OK;
}

// the Ruiz factors of the un-scaling epilogues: per LP when attached with the matrices, else the handle's shared ones
inline const void* batch_dcol(pdlp_handle h) { return h->bm.d_col ? h->bm.d_col : h->p.d_col; }
inline const void* batch_drow(pdlp_handle h) { return h->bm.d_row ? h->bm.d_row : h->p.d_row; }
inline int batch_dper(pdlp_handle h) { return h->bm.d_col ? 1 : 0; }

// the second set of partials (the adaptive rule needs two at once)
inline double* batch_part2(const pdlp_batch* b) { return b->part + (size_t)4 * BATCH_MAXG * b->Bp; }

template <typename T, int W, class Epi>
int batch_mv(pdlp_handle h, const pdlp_batch* b, bool transpose, const T* Vin, const Epi& epi, double* partials)
{
    const int rows = (int)(transpose ? h->p.n : h->p.m);
    const pdlp_problem& p = h->p;
    const int64_t* rp = transpose ? p.KT_rowptr : p.K_rowptr;
    const int32_t* ci = transpose ? p.KT_colidx : p.K_colidx;
    const dim3 grid(batch_grid(rows, W), b->Bp / W);
    if (h->bm.K_val) {
        const T* va = (const T*)(transpose ? h->bm.KT_val : h->bm.K_val);
        hipLaunchKernelGGL((k_batch_mv<T, W, true, Epi>), grid, dim3(BLOCK), 0, h->stream, rows, rp, ci, va, Vin, b->Bp, b->live, epi, partials);
    } else {
        const T* va = (const T*)(transpose ? p.KT_val : p.K_val);
        hipLaunchKernelGGL((k_batch_mv<T, W, false, Epi>), grid, dim3(BLOCK), 0, h->stream, rows, rp, ci, va, Vin, b->Bp, b->live, epi, partials);
    }
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// the same over every column b < B, frozen or not (the report, the plain product)
template <typename T, int W, class Epi>
int batch_mv_all(pdlp_handle h, const pdlp_batch* b, bool transpose, const T* Vin, const Epi& epi, double* partials)
{
    const int rows = (int)(transpose ? h->p.n : h->p.m);
    const pdlp_problem& p = h->p;
    const int64_t* rp = transpose ? p.KT_rowptr : p.K_rowptr;
    const int32_t* ci = transpose ? p.KT_colidx : p.K_colidx;
    const dim3 grid(batch_grid(rows, W), b->Bp / W);
    if (h->bm.K_val) {
        const T* va = (const T*)(transpose ? h->bm.KT_val : h->bm.K_val);
        hipLaunchKernelGGL((k_batch_mv_all<T, W, true, Epi>), grid, dim3(BLOCK), 0, h->stream, rows, rp, ci, va, Vin, b->Bp, b->B, epi, partials);
    } else {
        const T* va = (const T*)(transpose ? p.KT_val : p.K_val);
        hipLaunchKernelGGL((k_batch_mv_all<T, W, false, Epi>), grid, dim3(BLOCK), 0, h->stream, rows, rp, ci, va, Vin, b->Bp, b->B, epi, partials);
    }
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

int batch_finalize(pdlp_handle h, const pdlp_batch* b, const double* partials, int64_t rows, int na, int slot, int off)
{
    hipLaunchKernelGGL(k_batch_finalize, dim3(b->Bp * na), dim3(BLOCK), 0, h->stream, partials,
                       batch_grid(rows, b->W), b->Bp, na, b->out + (size_t)slot * b->Bp * 6, 6, off);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

#define BATCH_TRY(expr)                          \
    do {                                         \
        const int rc_ = (expr);                  \
        if (rc_ != PDLP_OK) return rc_;          \
    } while (0)

template <typename T, int W> int batch_iterate_w(pdlp_handle h, const pdlp_batch* b, int iters, bool adaptive, int64_t k0, const int64_t* k_start)
{
    const int ineq_end = (int)h->p.m_ineq;
    T *eta = (T*)b->eta, *omega = (T*)b->omega, *eta_sum = (T*)b->eta_sum, *wpend = (T*)b->wpend;
    for (int it = 0; it < iters; ++it) {
        if (adaptive) {
            BPrimal<T, true> ep{(T*)b->x, (T*)b->x_prev, (T*)b->xbar, (T*)b->x_sum, (const T*)b->c, (const T*)b->l, (const T*)b->u,
                                b->c_per_lp, b->l_per_lp, b->u_per_lp, eta, omega, wpend};
            BATCH_TRY((batch_mv<T, W>(h, b, true, (const T*)b->y, ep, nullptr)));
            BDual<T, true> ed{(T*)b->y, (T*)b->y_prev, (T*)b->y_sum, (T*)b->dy, (const T*)b->q, b->q_per_lp, eta, omega, wpend, ineq_end};
            BATCH_TRY((batch_mv<T, W>(h, b, false, (const T*)b->xbar, ed, b->part)));
            BDen<T> en{(const T*)b->x, (const T*)b->x_prev};
            BATCH_TRY((batch_mv<T, W>(h, b, true, (const T*)b->dy, en, batch_part2(b))));
            hipLaunchKernelGGL(k_batch_adapt<T>, dim3(b->Bp), dim3(BLOCK), 0, h->stream, b->Bp, b->live, b->part,
                               batch_grid(h->p.m, W), batch_part2(b), batch_grid(h->p.n, W), eta, omega, eta_sum, wpend, k0 + it + 1, k_start);
            HIP_TRY(hipGetLastError());
        } else {
            BPrimal<T, false> ep{(T*)b->x, (T*)b->x_prev, (T*)b->xbar, (T*)b->x_sum, (const T*)b->c, (const T*)b->l, (const T*)b->u,
                                 b->c_per_lp, b->l_per_lp, b->u_per_lp, eta, omega, wpend};
            BATCH_TRY((batch_mv<T, W>(h, b, true, (const T*)b->y, ep, nullptr)));
            BDual<T, false> ed{(T*)b->y, (T*)b->y_prev, (T*)b->y_sum, (T*)b->dy, (const T*)b->q, b->q_per_lp, eta, omega, wpend, ineq_end};
            BATCH_TRY((batch_mv<T, W>(h, b, false, (const T*)b->xbar, ed, nullptr)));
        }
    }
    if (!adaptive && iters > 0) {
        hipLaunchKernelGGL(k_batch_etasum<T>, dim3(grid_for(b->Bp)), dim3(BLOCK), 0, h->stream, b->Bp, b->live, (const T*)eta, eta_sum, iters);
        HIP_TRY(hipGetLastError());
    }
    return PDLP_OK;
}

template <typename T> int batch_iterate_t(pdlp_handle h, const pdlp_batch* b, int iters, int adaptive, int64_t k0, const int64_t* k_start)
{
    if (b->W == 8) return batch_iterate_w<T, 8>(h, b, iters, adaptive != 0, k0, k_start);
    if (b->W == 16) return batch_iterate_w<T, 16>(h, b, iters, adaptive != 0, k0, k_start);
    return batch_iterate_w<T, 32>(h, b, iters, adaptive != 0, k0, k_start);
}

template <typename T> int batch_average_t(pdlp_handle h, const pdlp_batch* b, int adaptive)
{
    const int64_t tn = h->p.n * (int64_t)b->Bp, tm = h->p.m * (int64_t)b->Bp;
    auto kern = adaptive ? k_batch_average<T, true> : k_batch_average<T, false>;
    hipLaunchKernelGGL(kern, dim3(grid_for(tn)), dim3(BLOCK), 0, h->stream, tn, b->Bp, b->live, (T*)b->x_sum, (const T*)b->x,
                       (T*)b->x_avg, (const T*)b->wpend, (const T*)b->eta_sum);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(kern, dim3(grid_for(tm)), dim3(BLOCK), 0, h->stream, tm, b->Bp, b->live, (T*)b->y_sum, (const T*)b->y,
                       (T*)b->y_avg, (const T*)b->wpend, (const T*)b->eta_sum);
    HIP_TRY(hipGetLastError());
    if (adaptive) {            // the pending terms are in the sums now
        hipLaunchKernelGGL(k_batch_zero_pending, dim3(grid_for(b->Bp)), dim3(BLOCK), 0, h->stream, b->Bp, b->live, b->wpend, (int)sizeof(T));
        HIP_TRY(hipGetLastError());
    }
    return PDLP_OK;
}

template <typename T, int W, bool U> int batch_kkt_w(pdlp_handle h, const pdlp_batch* b, int which, int slot)
{
    const T* X = (const T*)(which == PDLP_CUR ? b->x : which == PDLP_AVG ? b->x_avg : b->x_prev);
    const T* Y = (const T*)(which == PDLP_CUR ? b->y : which == PDLP_AVG ? b->y_avg : b->y_prev);
    BKktDual<T, U> ed{X, (const T*)b->c, (const T*)b->l, (const T*)b->u, b->c_per_lp, b->l_per_lp, b->u_per_lp, (const T*)batch_dcol(h),
                       batch_dper(h)};
    BATCH_TRY((batch_mv<T, W>(h, b, true, Y, ed, b->part)));
    BATCH_TRY(batch_finalize(h, b, b->part, h->p.n, 4, slot, 0));
    BKktPrimal<T, U> ep{Y, (const T*)b->q, b->q_per_lp, (const T*)batch_drow(h), batch_dper(h), (int)h->p.m_ineq};
    BATCH_TRY((batch_mv<T, W>(h, b, false, X, ep, batch_part2(b))));
    return batch_finalize(h, b, batch_part2(b), h->p.m, 2, slot, 4);
}

template <typename T> int batch_kkt_t(pdlp_handle h, const pdlp_batch* b, int which, int unscaled, int slot)
{
    if (unscaled) {
        if (b->W == 8) return batch_kkt_w<T, 8, true>(h, b, which, slot);
        if (b->W == 16) return batch_kkt_w<T, 16, true>(h, b, which, slot);
        return batch_kkt_w<T, 32, true>(h, b, which, slot);
    }
    if (b->W == 8) return batch_kkt_w<T, 8, false>(h, b, which, slot);
    if (b->W == 16) return batch_kkt_w<T, 16, false>(h, b, which, slot);
    return batch_kkt_w<T, 32, false>(h, b, which, slot);
}

// the report of every LP b < B: the two products of a KKT pass over all columns, lam and K x stored, the sums of columns b < B
// into out[slot] (padding columns of rc, act and out are never written: the finalize launch ends at column B)
template <typename T, int W, bool U> int batch_report_w(pdlp_handle h, const pdlp_batch* b, int which, int slot, void* rc, void* act)
{
    const T* X = (const T*)(which == PDLP_CUR ? b->x : which == PDLP_AVG ? b->x_avg : b->x_prev);
    const T* Y = (const T*)(which == PDLP_CUR ? b->y : which == PDLP_AVG ? b->y_avg : b->y_prev);
    const pdlp_problem& p = h->p;
    double* out = b->out + (size_t)slot * b->Bp * 6;
    BReportDual<T, U> ed{{X, (const T*)b->c, (const T*)b->l, (const T*)b->u, b->c_per_lp, b->l_per_lp, b->u_per_lp,
                          (const T*)batch_dcol(h), batch_dper(h)}, (T*)rc};
    BATCH_TRY((batch_mv_all<T, W>(h, b, true, Y, ed, b->part)));
    hipLaunchKernelGGL(k_batch_finalize, dim3(b->B * 4), dim3(BLOCK), 0, h->stream, (const double*)b->part, batch_grid(p.n, W), b->Bp, 4, out, 6, 0);
    BReportPrimal<T, U> ep{{Y, (const T*)b->q, b->q_per_lp, (const T*)batch_drow(h), batch_dper(h), (int)p.m_ineq}, (T*)act};
    BATCH_TRY((batch_mv_all<T, W>(h, b, false, X, ep, batch_part2(b))));
    hipLaunchKernelGGL(k_batch_finalize, dim3(b->B * 2), dim3(BLOCK), 0, h->stream, (const double*)batch_part2(b), batch_grid(p.m, W), b->Bp, 2, out, 6, 4);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

template <typename T> int batch_report_t(pdlp_handle h, const pdlp_batch* b, int which, int unscaled, int slot, void* rc, void* act)
{
    if (unscaled) {
        if (b->W == 8) return batch_report_w<T, 8, true>(h, b, which, slot, rc, act);
        if (b->W == 16) return batch_report_w<T, 16, true>(h, b, which, slot, rc, act);
        return batch_report_w<T, 32, true>(h, b, which, slot, rc, act);
    }
    if (b->W == 8) return batch_report_w<T, 8, false>(h, b, which, slot, rc, act);
    if (b->W == 16) return batch_report_w<T, 16, false>(h, b, which, slot, rc, act);
    return batch_report_w<T, 32, false>(h, b, which, slot, rc, act);
}

// admission: one launch per side -- the n rows (c, l, u, x and the LP's scalars), the m rows (q, y), the nnz items (both value
// populations, when matrices are attached)
template <typename T> int batch_admit_t(pdlp_handle h, const pdlp_batch* b, int count, const int32_t* cols, const int32_t* ids,
                                        const pdlp_batch_feed* f)
{
    const int64_t n = h->p.n, m = h->p.m;
    T* const none = nullptr;
    hipLaunchKernelGGL(k_batch_admit<T>, dim3(grid_for(n * count)), dim3(BLOCK), 0, h->stream, n, count, cols, ids, b->Bp, f->N,
                       f->c ? (T*)b->c : none, (const T*)f->c, f->l ? (T*)b->l : none, (const T*)f->l, f->u ? (T*)b->u : none,
                       (const T*)f->u, (T*)b->x, (T*)b->x_last, (T*)b->x_sum, (const T*)f->x0, (T*)b->eta, (T*)b->omega, (T*)b->eta_sum,
                       (T*)b->wpend, (const T*)f->eta, (const T*)f->omega);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_batch_admit<T>, dim3(grid_for(m * count)), dim3(BLOCK), 0, h->stream, m, count, cols, ids, b->Bp, f->N,
                       f->q ? (T*)b->q : none, (const T*)f->q, none, (const T*)nullptr, none, (const T*)nullptr, (T*)b->y, (T*)b->y_last,
                       (T*)b->y_sum, (const T*)f->y0, none, none, none, none, (const T*)nullptr, (const T*)nullptr);
    HIP_TRY(hipGetLastError());
    if (f->K_val) {
        const int64_t nnz = h->nnz;
        hipLaunchKernelGGL(k_batch_admit<T>, dim3(grid_for(nnz * count)), dim3(BLOCK), 0, h->stream, nnz, count, cols, ids, b->Bp, f->N,
                           (T*)h->bm.K_val, (const T*)f->K_val, (T*)h->bm.KT_val, (const T*)f->KT_val, none, (const T*)nullptr, none, none,
                           none, (const T*)nullptr, none, none, none, none, (const T*)nullptr, (const T*)nullptr);
        HIP_TRY(hipGetLastError());
    }
    return PDLP_OK;
}

// retirement: the report of the listed columns, stored into the caller's [len][N] arrays; the sums through the report's tree
template <typename T, int W, bool U>
int batch_retire_w(pdlp_handle h, const pdlp_batch* b, int count, const int32_t* cols, const int32_t* ids, int which, int slot,
                   void* Xo, void* Yo, void* rc, void* act, int N)
{
    const T* X = (const T*)(which == PDLP_CUR ? b->x : which == PDLP_AVG ? b->x_avg : b->x_prev);
    const T* Y = (const T*)(which == PDLP_CUR ? b->y : which == PDLP_AVG ? b->y_avg : b->y_prev);
    const pdlp_problem& p = h->p;
    double* out = b->out + (size_t)slot * b->Bp * 6;
    const bool per = h->bm.K_val != nullptr;
    for (int side = 0; side < 2; ++side) {      // 0: rows of K' (x, lam, four sums), 1: rows of K (y, K x, two sums)
        const int rows = (int)(side == 0 ? p.n : p.m);
        const int64_t* rp = side == 0 ? p.KT_rowptr : p.K_rowptr;
        const int32_t* ci = side == 0 ? p.KT_colidx : p.K_colidx;
        const T* va = (const T*)(per ? (side == 0 ? h->bm.KT_val : h->bm.K_val) : (side == 0 ? p.KT_val : p.K_val));
        const dim3 grid(batch_grid(rows, W), b->Bp / W);
        double* part = side == 0 ? b->part : batch_part2(b);
        if (side == 0) {
            BRetireDual<T, U> e{{X, (const T*)b->c, (const T*)b->l, (const T*)b->u, b->c_per_lp, b->l_per_lp, b->u_per_lp,
                                 (const T*)batch_dcol(h), batch_dper(h)}, (T*)Xo, (T*)rc, N, -1};
            if (per) hipLaunchKernelGGL((k_batch_mv_cols<T, W, true, BRetireDual<T, U>>), grid, dim3(BLOCK), 0, h->stream, rows, rp, ci, va, Y, b->Bp, count, cols, ids, N, e, part);
            else hipLaunchKernelGGL((k_batch_mv_cols<T, W, false, BRetireDual<T, U>>), grid, dim3(BLOCK), 0, h->stream, rows, rp, ci, va, Y, b->Bp, count, cols, ids, N, e, part);
        } else {
            BRetirePrimal<T, U> e{{Y, (const T*)b->q, b->q_per_lp, (const T*)batch_drow(h), batch_dper(h), (int)p.m_ineq}, (T*)Yo, (T*)act, N, -1};
            if (per) hipLaunchKernelGGL((k_batch_mv_cols<T, W, true, BRetirePrimal<T, U>>), grid, dim3(BLOCK), 0, h->stream, rows, rp, ci, va, X, b->Bp, count, cols, ids, N, e, part);
            else hipLaunchKernelGGL((k_batch_mv_cols<T, W, false, BRetirePrimal<T, U>>), grid, dim3(BLOCK), 0, h->stream, rows, rp, ci, va, X, b->Bp, count, cols, ids, N, e, part);
        }
        HIP_TRY(hipGetLastError());
        const int na = side == 0 ? 4 : 2;
        hipLaunchKernelGGL(k_batch_finalize_cols, dim3(count * na), dim3(BLOCK), 0, h->stream, (const double*)part, batch_grid(rows, W), b->Bp,
                           na, cols, out, 6, side == 0 ? 0 : 4);
        HIP_TRY(hipGetLastError());
    }
    return PDLP_OK;
}

template <typename T>
int batch_retire_t(pdlp_handle h, const pdlp_batch* b, int count, const int32_t* cols, const int32_t* ids, int which, int unscaled,
                   int slot, void* Xo, void* Yo, void* rc, void* act, int N)
{
    if (unscaled) {
        if (b->W == 8) return batch_retire_w<T, 8, true>(h, b, count, cols, ids, which, slot, Xo, Yo, rc, act, N);
        if (b->W == 16) return batch_retire_w<T, 16, true>(h, b, count, cols, ids, which, slot, Xo, Yo, rc, act, N);
        return batch_retire_w<T, 32, true>(h, b, count, cols, ids, which, slot, Xo, Yo, rc, act, N);
    }
    if (b->W == 8) return batch_retire_w<T, 8, false>(h, b, count, cols, ids, which, slot, Xo, Yo, rc, act, N);
    if (b->W == 16) return batch_retire_w<T, 16, false>(h, b, count, cols, ids, which, slot, Xo, Yo, rc, act, N);
    return batch_retire_w<T, 32, false>(h, b, count, cols, ids, which, slot, Xo, Yo, rc, act, N);
}

template <typename T> int batch_product_t(pdlp_handle h, const pdlp_batch* b, int transpose, const void* Vin, void* Vout)
{
    BStore<T> es{(T*)Vout};
    if (b->W == 8) return batch_mv_all<T, 8>(h, b, transpose != 0, (const T*)Vin, es, nullptr);
    if (b->W == 16) return batch_mv_all<T, 16>(h, b, transpose != 0, (const T*)Vin, es, nullptr);
    return batch_mv_all<T, 32>(h, b, transpose != 0, (const T*)Vin, es, nullptr);
}

template <typename T, int W> int batch_restart_w(pdlp_handle h, const pdlp_batch* b, int slot)
{
    const dim3 gn(batch_grid(h->p.n, W), b->Bp / W), gm(batch_grid(h->p.m, W), b->Bp / W);
    hipLaunchKernelGGL((k_batch_restart<T, W>), gn, dim3(BLOCK), 0, h->stream, (int)h->p.n, b->Bp, b->action, (T*)b->x,
                       (const T*)b->x_avg, (T*)b->x_sum, (T*)b->x_last, (T*)b->eta_sum, (T*)b->wpend, b->part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_batch_restart<T, W>), gm, dim3(BLOCK), 0, h->stream, (int)h->p.m, b->Bp, b->action, (T*)b->y,
                       (const T*)b->y_avg, (T*)b->y_sum, (T*)b->y_last, (T*)nullptr, (T*)nullptr, batch_part2(b));
    HIP_TRY(hipGetLastError());
    BATCH_TRY(batch_finalize(h, b, b->part, h->p.n, 1, slot, 0));
    return batch_finalize(h, b, batch_part2(b), h->p.m, 1, slot, 1);
}

template <typename T> int batch_restart_t(pdlp_handle h, const pdlp_batch* b, int slot)
{
    if (b->W == 8) return batch_restart_w<T, 8>(h, b, slot);
    if (b->W == 16) return batch_restart_w<T, 16>(h, b, slot);
    return batch_restart_w<T, 32>(h, b, slot);
}

#undef BATCH_TRY

}  // namespace

int pdlp_batch_iterate_from(pdlp_handle h, const pdlp_batch* b, int iters, int adaptive, int64_t k0, const int64_t* k_start)
{
    if (iters < 0 || k0 < 0) return PDLP_ERR_INVALID;
    const int rc = batch_check(h, b);
    if (rc != PDLP_OK) return rc;
    Range range("pdlp: batch iterations", h->stream);
    return DISPATCH(h, batch_iterate_t, h, b, iters, adaptive, k0, k_start);
}

int pdlp_batch_iterate(pdlp_handle h, const pdlp_batch* b, int iters, int adaptive, int64_t k0)
{
    return pdlp_batch_iterate_from(h, b, iters, adaptive, k0, nullptr);
}

int pdlp_batch_admit(pdlp_handle h, const pdlp_batch* b, int count, const int32_t* cols, const int32_t* ids, const pdlp_batch_feed* f)
{
    const int rc = batch_check(h, b);
    if (rc != PDLP_OK) return rc;
    if (!f || !cols || !ids || count < 1 || count > b->Bp || f->N < 1 || !f->eta || !f->omega) return PDLP_ERR_INVALID;
    // a vector is fed exactly where the batch holds a column of it per LP, the values exactly where matrices are attached
    if ((f->c != nullptr) != (b->c_per_lp != 0) || (f->q != nullptr) != (b->q_per_lp != 0) || (f->l != nullptr) != (b->l_per_lp != 0) ||
        (f->u != nullptr) != (b->u_per_lp != 0))
        return PDLP_ERR_INVALID;
    if ((f->K_val != nullptr) != (f->KT_val != nullptr) || (f->K_val != nullptr) != (h->bm.K_val != nullptr)) return PDLP_ERR_INVALID;
    Range range("pdlp: batch admission", h->stream);
    return DISPATCH(h, batch_admit_t, h, b, count, cols, ids, f);
}

int pdlp_batch_retire(pdlp_handle h, const pdlp_batch* b, int count, const int32_t* cols, const int32_t* ids, int which, int unscaled,
                      int slot, void* X_out, void* Y_out, void* rc_out, void* act_out, int N)
{
    if ((which != PDLP_CUR && which != PDLP_AVG && which != PDLP_PREV) || slot < 0 || slot > 2) return PDLP_ERR_INVALID;
    const int r = batch_check(h, b);
    if (r != PDLP_OK) return r;
    if (!cols || !ids || count < 1 || count > b->Bp || !X_out || !Y_out || N < 1) return PDLP_ERR_INVALID;
    if (unscaled && (!batch_dcol(h) || !batch_drow(h))) return PDLP_ERR_STATE;
    Range range("pdlp: batch retirement", h->stream);
    return DISPATCH(h, batch_retire_t, h, b, count, cols, ids, which, unscaled, slot, X_out, Y_out, rc_out, act_out, N);
}

int pdlp_batch_average(pdlp_handle h, const pdlp_batch* b, int adaptive)
{
    const int rc = batch_check(h, b);
    if (rc != PDLP_OK) return rc;
    return DISPATCH(h, batch_average_t, h, b, adaptive);
}

int pdlp_batch_kkt(pdlp_handle h, const pdlp_batch* b, int which, int unscaled, int slot)
{
    if ((which != PDLP_CUR && which != PDLP_AVG && which != PDLP_PREV) || slot < 0 || slot > 2) return PDLP_ERR_INVALID;
    const int rc = batch_check(h, b);
    if (rc != PDLP_OK) return rc;
    if (unscaled && (!batch_dcol(h) || !batch_drow(h))) return PDLP_ERR_STATE;
    Range range("pdlp: batch KKT pass", h->stream);
    return DISPATCH(h, batch_kkt_t, h, b, which, unscaled, slot);
}

int pdlp_batch_report(pdlp_handle h, const pdlp_batch* b, int which, int unscaled, int slot, void* rc, void* act)
{
    if ((which != PDLP_CUR && which != PDLP_AVG && which != PDLP_PREV) || slot < 0 || slot > 2) return PDLP_ERR_INVALID;
    const int r = batch_check(h, b);
    if (r != PDLP_OK) return r;
    if (unscaled && (!batch_dcol(h) || !batch_drow(h))) return PDLP_ERR_STATE;
    Range range("pdlp: batch solution report", h->stream);
    return DISPATCH(h, batch_report_t, h, b, which, unscaled, slot, rc, act);
}

int pdlp_batch_restart(pdlp_handle h, const pdlp_batch* b, int slot)
{
    if (slot < 0 || slot > 2) return PDLP_ERR_INVALID;
    const int rc = batch_check(h, b);
    if (rc != PDLP_OK) return rc;
    return DISPATCH(h, batch_restart_t, h, b, slot);
}

int pdlp_batch_attach_matrices(pdlp_handle h, int Bp, const void* K_valB, const void* KT_valB, const void* d_colB, const void* d_rowB)
{
    if (!h) return PDLP_ERR_INVALID;
    if (!K_valB && !KT_valB) {                                  // detach: back to the handle's shared matrix and factors
        if (d_colB || d_rowB) return PDLP_ERR_INVALID;
        h->bm = pdlp_solver::BatchMatrices();
        return PDLP_OK;
    }
    if (!K_valB || !KT_valB || Bp < 8 || Bp % 8 != 0 || (d_colB == nullptr) != (d_rowB == nullptr)) return PDLP_ERR_INVALID;
    if (h->nl != h->p.n || h->ml != h->p.m || h->mixed || h->delta) return PDLP_ERR_STATE;     // single GPU, one precision
    h->bm.Bp = Bp;
    h->bm.K_val = K_valB; h->bm.KT_val = KT_valB;
    h->bm.d_col = d_colB; h->bm.d_row = d_rowB;
    return PDLP_OK;
}

int pdlp_batch_product(pdlp_handle h, const pdlp_batch* b, int transpose, const void* Vin, void* Vout)
{
    if (!Vin || !Vout || Vin == Vout) return PDLP_ERR_INVALID;
    const int rc = batch_check(h, b);
    if (rc != PDLP_OK) return rc;
    Range range("pdlp: batch product", h->stream);
    return DISPATCH(h, batch_product_t, h, b, transpose, Vin, Vout);
}
