// pdlp_batch_host.inc -- host side of the batched solves (pdlp_batch_*, include/pdlp_hip.h): launch shapes and the C entry points.
// Part of pdlp_hip.hip (included at file scope after the other entry points; not a translation unit of its own).
// Kernels: pdlp_kernel_batch.inc.  Every population product is one batch_launch of k_batch_mv, instantiated per (dtype, W, shared
// or per-LP matrix values, column selector, epilogue) -- batch_dispatch turns the batch's dtype and W into those constants; every
// other flag (shared or per-LP vectors, the iteration count) is a launch argument.  With matrices attached
// (pdlp_batch_attach_matrices) every product reads the per-LP values and the un-scaling epilogues the per-LP Ruiz factors.  The
// report and retirement are one body (batch_report_w) under two selectors.
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
    if (!whole_problem(h) || h->mixed || h->delta) return PDLP_ERR_STATE;     // single GPU, one precision
    if (h->obj_diag || h->obj_mat.on) return PDLP_ERR_STATE;      // (the batch kernels know the linear objective only)
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

// The element type and W of a batch as compile-time constants, f(T(), integral_constant<int, W>()), and a flag beside them,
// f(T(), integral_constant<int, W>(), bool_constant<flag>()): what DISPATCH is for the element type alone.  Use: TYPE(t), VAL(w)
template <class F> int batch_dispatch(pdlp_handle h, const pdlp_batch* b, F f)
{
    auto width = [&](auto t) {
        if (b->W == 8) return f(t, std::integral_constant<int, 8>());
        if (b->W == 16) return f(t, std::integral_constant<int, 16>());
        return f(t, std::integral_constant<int, 32>());
    };
    return h->p.dtype == PDLP_F32 ? width(float()) : width(double());
}
template <class F> int batch_dispatch(pdlp_handle h, const pdlp_batch* b, int flag, F f)
{
    return batch_dispatch(h, b, [&](auto t, auto w) { return flag ? f(t, w, std::true_type()) : f(t, w, std::false_type()); });
}
#define TYPE(t) decltype(t)
#define VAL(c) decltype(c)::value

// one product launch: K (or K' with `transpose`) times the population Vin over the columns `sel` picks, with every LP's own
// values when matrices are attached
template <typename T, int W, class Sel, class Epi>
int batch_launch(pdlp_handle h, const pdlp_batch* b, bool transpose, const T* Vin, const Sel& sel, const Epi& epi, double* partials)
{
    const int rows = (int)(transpose ? h->p.n : h->p.m);
    const pdlp_problem& p = h->p;
    const int64_t* rp = transpose ? p.KT_rowptr : p.K_rowptr;
    const int32_t* ci = transpose ? p.KT_colidx : p.K_colidx;
    const dim3 grid(batch_grid(rows, W), b->Bp / W);
    if (h->bm.K_val) {
        const T* va = (const T*)(transpose ? h->bm.KT_val : h->bm.K_val);
        hipLaunchKernelGGL((k_batch_mv<T, W, true, Sel, Epi>), grid, dim3(BLOCK), 0, h->stream, rows, rp, ci, va, Vin, b->Bp, sel, epi, partials);
    } else {
        const T* va = (const T*)(transpose ? p.KT_val : p.K_val);
        hipLaunchKernelGGL((k_batch_mv<T, W, false, Sel, Epi>), grid, dim3(BLOCK), 0, h->stream, rows, rp, ci, va, Vin, b->Bp, sel, epi, partials);
    }
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// the sums of `count` columns into out[slot]: every column of the population, or the listed ones
int batch_finalize(pdlp_handle h, const pdlp_batch* b, const double* partials, int64_t rows, int na, int slot, int off, int count,
                   const int32_t* cols = nullptr, const int32_t* ids = nullptr, int N = 0)
{
    hipLaunchKernelGGL(k_batch_finalize, dim3(count * na), dim3(BLOCK), 0, h->stream, partials, batch_grid(rows, b->W), b->Bp, na,
                       cols, ids, N, b->out + (size_t)slot * b->Bp * 6, 6, off);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// the arguments of a pass over an iterate: `which` and the slot of its sums; the Ruiz factors an un-scaled pass divides by
int batch_check_pass(pdlp_handle h, const pdlp_batch* b, int which, int slot)
{
    if ((which != PDLP_CUR && which != PDLP_AVG && which != PDLP_PREV) || slot < 0 || slot > 2) return PDLP_ERR_INVALID;
    return batch_check(h, b);
}
int batch_check_unscaled(pdlp_handle h, int unscaled) { return unscaled && (!batch_dcol(h) || !batch_drow(h)) ? PDLP_ERR_STATE : PDLP_OK; }

// the iterate `which` of the batch behind the KKT epilogues of its two sides
template <typename T, bool U> BKktDual<T, U> batch_kkt_dual(pdlp_handle h, const pdlp_batch* b, int which)
{
    const void* X = which == PDLP_CUR ? b->x : which == PDLP_AVG ? b->x_avg : b->x_prev;
    return {(const T*)X, (const T*)b->c, (const T*)b->l, (const T*)b->u, b->c_per_lp, b->l_per_lp, b->u_per_lp, (const T*)batch_dcol(h), batch_dper(h)};
}
template <typename T, bool U> BKktPrimal<T, U> batch_kkt_primal(pdlp_handle h, const pdlp_batch* b, int which)
{
    const void* Y = which == PDLP_CUR ? b->y : which == PDLP_AVG ? b->y_avg : b->y_prev;
    return {(const T*)Y, (const T*)b->q, b->q_per_lp, (const T*)batch_drow(h), batch_dper(h), (int)h->p.m_ineq};
}

#define BATCH_TRY(expr)                          \
    do {                                         \
        const int rc_ = (expr);                  \
        if (rc_ != PDLP_OK) return rc_;          \
    } while (0)

template <typename T, int W, bool ADAPT> int batch_iterate_w(pdlp_handle h, const pdlp_batch* b, int iters, int64_t k0, const int64_t* k_start)
{
    const BSelLive live{b->live};
    T *eta = (T*)b->eta, *omega = (T*)b->omega, *eta_sum = (T*)b->eta_sum, *wpend = (T*)b->wpend;
    const BPrimal<T, ADAPT> ep{(T*)b->x, (T*)b->x_prev, (T*)b->xbar, (T*)b->x_sum, (const T*)b->c, (const T*)b->l, (const T*)b->u,
                               b->c_per_lp, b->l_per_lp, b->u_per_lp, eta, omega, wpend};
    const BDual<T, ADAPT> ed{(T*)b->y, (T*)b->y_prev, (T*)b->y_sum, (T*)b->dy, (const T*)b->q, b->q_per_lp, eta, omega, wpend, (int)h->p.m_ineq};
    const BDen<T> en{(const T*)b->x, (const T*)b->x_prev};
    for (int it = 0; it < iters; ++it) {
        BATCH_TRY((batch_launch<T, W>(h, b, true, (const T*)b->y, live, ep, nullptr)));
        BATCH_TRY((batch_launch<T, W>(h, b, false, (const T*)b->xbar, live, ed, ADAPT ? b->part : nullptr)));
        if (ADAPT) {
            BATCH_TRY((batch_launch<T, W>(h, b, true, (const T*)b->dy, live, en, batch_part2(b))));
            hipLaunchKernelGGL(k_batch_adapt<T>, dim3(b->Bp), dim3(BLOCK), 0, h->stream, b->Bp, b->live, b->part,
                               batch_grid(h->p.m, W), batch_part2(b), batch_grid(h->p.n, W), eta, omega, eta_sum, wpend, k0 + it + 1, k_start);
            HIP_TRY(hipGetLastError());
        }
    }
    if (!ADAPT && iters > 0) {
        hipLaunchKernelGGL(k_batch_etasum<T>, dim3(grid_for(b->Bp)), dim3(BLOCK), 0, h->stream, b->Bp, b->live, (const T*)eta, eta_sum, iters);
        HIP_TRY(hipGetLastError());
    }
    return PDLP_OK;
}

// the restarted, reflected Halpern iteration: the two products of batch_iterate_w under BHalpernPrimal / BHalpernDual; the iterate
// is updated in place (x, y), the candidate goes to x_avg / y_avg, the anchor is x_last / y_last
template <typename T, int W> int batch_halpern_w(pdlp_handle h, const pdlp_batch* b, int iters, const int64_t* t_since)
{
    const BSelLive live{b->live};
    const T *eta = (const T*)b->eta, *omega = (const T*)b->omega;
    for (int it = 0; it < iters; ++it) {
        const BHalpernWeights<T> w{t_since, (int64_t)it};
        const BHalpernPrimal<T> ep{(T*)b->x, (T*)b->xbar, (T*)b->x_avg, (const T*)b->x_last, (const T*)b->c, (const T*)b->l,
                                   (const T*)b->u, b->c_per_lp, b->l_per_lp, b->u_per_lp, eta, omega, w};
        const BHalpernDual<T> ed{(T*)b->y, (T*)b->y_avg, (const T*)b->y_last, (const T*)b->q, b->q_per_lp, eta, omega, (int)h->p.m_ineq, w};
        BATCH_TRY((batch_launch<T, W>(h, b, true, (const T*)b->y, live, ep, nullptr)));
        BATCH_TRY((batch_launch<T, W>(h, b, false, (const T*)b->xbar, live, ed, nullptr)));
    }
    return PDLP_OK;
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
    const BSelLive live{b->live};
    const BKktDual<T, U> ed = batch_kkt_dual<T, U>(h, b, which);
    const BKktPrimal<T, U> ep = batch_kkt_primal<T, U>(h, b, which);
    BATCH_TRY((batch_launch<T, W>(h, b, true, ep.Y, live, ed, b->part)));
    BATCH_TRY(batch_finalize(h, b, b->part, h->p.n, 4, slot, 0, b->Bp));
    BATCH_TRY((batch_launch<T, W>(h, b, false, ed.X, live, ep, batch_part2(b))));
    return batch_finalize(h, b, batch_part2(b), h->p.m, 2, slot, 4, b->Bp);
}

// The solution report of the columns `sel` picks: the two products of a KKT pass with lam and K x stored (and the iterate, where
// Xo / Yo are given) at column `id` of the [len][N] arrays, the six sums of the `count` columns into out[slot].  pdlp_batch_report:
// every LP b < B into [len][Bp] arrays, column b (padding columns of rc, act and out are never written: the finalize launch ends
// at column B); pdlp_batch_retire: the listed columns into the caller's results.
template <typename T, int W, bool U, class Sel>
int batch_report_w(pdlp_handle h, const pdlp_batch* b, int which, int slot, const Sel& sel, int count, const int32_t* cols,
                   const int32_t* ids, void* Xo, void* Yo, void* rc, void* act, int N)
{
    const BReportDual<T, U> ed{batch_kkt_dual<T, U>(h, b, which), (T*)Xo, (T*)rc, N};
    const BReportPrimal<T, U> ep{batch_kkt_primal<T, U>(h, b, which), (T*)Yo, (T*)act, N};
    BATCH_TRY((batch_launch<T, W>(h, b, true, ep.kkt.Y, sel, ed, b->part)));
    BATCH_TRY(batch_finalize(h, b, b->part, h->p.n, 4, slot, 0, count, cols, ids, N));
    BATCH_TRY((batch_launch<T, W>(h, b, false, ed.kkt.X, sel, ep, batch_part2(b))));
    return batch_finalize(h, b, batch_part2(b), h->p.m, 2, slot, 4, count, cols, ids, N);
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

template <typename T, int W> int batch_restart_w(pdlp_handle h, const pdlp_batch* b, int slot)
{
    const dim3 gn(batch_grid(h->p.n, W), b->Bp / W), gm(batch_grid(h->p.m, W), b->Bp / W);
    hipLaunchKernelGGL((k_batch_restart<T, W>), gn, dim3(BLOCK), 0, h->stream, (int)h->p.n, b->Bp, b->action, (T*)b->x,
                       (const T*)b->x_avg, (T*)b->x_sum, (T*)b->x_last, (T*)b->eta_sum, (T*)b->wpend, b->part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_batch_restart<T, W>), gm, dim3(BLOCK), 0, h->stream, (int)h->p.m, b->Bp, b->action, (T*)b->y,
                       (const T*)b->y_avg, (T*)b->y_sum, (T*)b->y_last, (T*)nullptr, (T*)nullptr, batch_part2(b));
    HIP_TRY(hipGetLastError());
    BATCH_TRY(batch_finalize(h, b, b->part, h->p.n, 1, slot, 0, b->Bp));
    return batch_finalize(h, b, batch_part2(b), h->p.m, 1, slot, 1, b->Bp);
}

#undef BATCH_TRY

}  // namespace

int pdlp_batch_iterate_from(pdlp_handle h, const pdlp_batch* b, int iters, int adaptive, int64_t k0, const int64_t* k_start)
{
    if (iters < 0 || k0 < 0) return PDLP_ERR_INVALID;
    const int rc = batch_check(h, b);
    if (rc != PDLP_OK) return rc;
    Range range("pdlp: batch iterations", h->stream);
    return batch_dispatch(h, b, adaptive, [&](auto t, auto w, auto a) { return batch_iterate_w<TYPE(t), VAL(w), VAL(a)>(h, b, iters, k0, k_start); });
}

int pdlp_batch_iterate(pdlp_handle h, const pdlp_batch* b, int iters, int adaptive, int64_t k0)
{
    return pdlp_batch_iterate_from(h, b, iters, adaptive, k0, nullptr);
}

int pdlp_batch_halpern_iterate(pdlp_handle h, const pdlp_batch* b, int iters, const int64_t* t_since)
{
    if (iters < 0 || !t_since) return PDLP_ERR_INVALID;
    const int rc = batch_check(h, b);
    if (rc != PDLP_OK) return rc;
    Range range("pdlp: batch Halpern iterations", h->stream);
    return batch_dispatch(h, b, [&](auto t, auto w) { return batch_halpern_w<TYPE(t), VAL(w)>(h, b, iters, t_since); });
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
    int r = batch_check_pass(h, b, which, slot);
    if (r != PDLP_OK) return r;
    if (!cols || !ids || count < 1 || count > b->Bp || !X_out || !Y_out || N < 1) return PDLP_ERR_INVALID;
    if ((r = batch_check_unscaled(h, unscaled)) != PDLP_OK) return r;
    Range range("pdlp: batch retirement", h->stream);
    const BSelList sel{count, cols, ids, b->Bp, N};
    return batch_dispatch(h, b, unscaled, [&](auto t, auto w, auto u) {
        return batch_report_w<TYPE(t), VAL(w), VAL(u)>(h, b, which, slot, sel, count, cols, ids, X_out, Y_out, rc_out, act_out, N);
    });
}

int pdlp_batch_average(pdlp_handle h, const pdlp_batch* b, int adaptive)
{
    const int rc = batch_check(h, b);
    if (rc != PDLP_OK) return rc;
    return DISPATCH(h, batch_average_t, h, b, adaptive);
}

int pdlp_batch_kkt(pdlp_handle h, const pdlp_batch* b, int which, int unscaled, int slot)
{
    int rc = batch_check_pass(h, b, which, slot);
    if (rc != PDLP_OK || (rc = batch_check_unscaled(h, unscaled)) != PDLP_OK) return rc;
    Range range("pdlp: batch KKT pass", h->stream);
    return batch_dispatch(h, b, unscaled, [&](auto t, auto w, auto u) { return batch_kkt_w<TYPE(t), VAL(w), VAL(u)>(h, b, which, slot); });
}

int pdlp_batch_report(pdlp_handle h, const pdlp_batch* b, int which, int unscaled, int slot, void* rc, void* act)
{
    int r = batch_check_pass(h, b, which, slot);
    if (r != PDLP_OK || (r = batch_check_unscaled(h, unscaled)) != PDLP_OK) return r;
    Range range("pdlp: batch solution report", h->stream);
    const BSelAll sel{b->B};
    return batch_dispatch(h, b, unscaled, [&](auto t, auto w, auto u) {
        return batch_report_w<TYPE(t), VAL(w), VAL(u)>(h, b, which, slot, sel, b->B, nullptr, nullptr, nullptr, nullptr, rc, act, b->Bp);
    });
}

int pdlp_batch_restart(pdlp_handle h, const pdlp_batch* b, int slot)
{
    if (slot < 0 || slot > 2) return PDLP_ERR_INVALID;
    const int rc = batch_check(h, b);
    if (rc != PDLP_OK) return rc;
    return batch_dispatch(h, b, [&](auto t, auto w) { return batch_restart_w<TYPE(t), VAL(w)>(h, b, slot); });
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
    if (!whole_problem(h) || h->mixed || h->delta || h->obj_diag || h->obj_mat.on) return PDLP_ERR_STATE;     // single GPU, one precision, linear objective
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
    return batch_dispatch(h, b, [&](auto t, auto w) {
        using T = TYPE(t);
        return batch_launch<T, VAL(w)>(h, b, transpose != 0, (const T*)Vin, BSelAll{b->B}, BStore<T>{(T*)Vout}, nullptr);
    });
}
#undef TYPE
#undef VAL
