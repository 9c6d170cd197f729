// pdlp_kkt.inc -- everything a restart check evaluates: the KKT pass (kkt_local_*: six sums of a candidate, from products or from
// the running sums), the solution report, the finish of the sums in the working precision, the running average's flush and
// division, the restart distance, infeasibility detection and the power iteration; and pdlp_restart, which adopts a candidate
// together with the products its KKT pass left behind.
// Part of pdlp_hip.hip (included at file scope; not a translation unit of its own).  Needs: pdlp_products.inc and what is before it.
// ------------------------------------------------------------------------------------------------
namespace {

// the functors of a KKT pass and of a report: the constraint side with q_upper when the handle has two-sided rows (RANGED), the
// variable side with d when it has a diagonal quadratic objective (QUAD); with a sparse quadratic objective the variable side reads
// the gradient g = c + Q x of the evaluated point where it reads c (obj_linear: kkt_pass_begin has formed it)
template <typename T, bool UNSCALE, bool RANGED> KktPrimalEpi<T, UNSCALE, RANGED> kkt_primal_epi(pdlp_handle h, int ix, const T* drow, T* kx_out)
{
    KktPrimalEpi<T, UNSCALE, RANGED> ep{yloc<T>(h, ix), (const T*)h->p.q, drow, kx_out, h->ineq_end};
    set_optional(ep.upper, h);
    return ep;
}
template <typename T, bool UNSCALE, bool QUAD> KktDualEpi<T, UNSCALE, QUAD> kkt_dual_epi(pdlp_handle h, int ix, const T* dcol, T* kty_out)
{
    KktDualEpi<T, UNSCALE, QUAD> ed{xloc<T>(h, ix), obj_linear<T>(h), (const T*)h->p.l, (const T*)h->p.u, dcol, kty_out};
    set_optional(ed.diag, h);
    return ed;
}
template <typename T, bool UNSCALE, bool RANGED> ReportPrimalEpi<T, UNSCALE, RANGED> report_primal_epi(pdlp_handle h, int ix, const T* drow, T* buf)
{
    ReportPrimalEpi<T, UNSCALE, RANGED> ep{buf, yloc<T>(h, ix), (const T*)h->p.q, drow, h->ineq_end};
    set_optional(ep.upper, h);
    return ep;
}
template <typename T, bool UNSCALE, bool QUAD> ReportDualEpi<T, UNSCALE, QUAD> report_dual_epi(pdlp_handle h, int ix, const T* dcol, T* buf)
{
    ReportDualEpi<T, UNSCALE, QUAD> ed{buf, xloc<T>(h, ix), obj_linear<T>(h), (const T*)h->p.l, (const T*)h->p.u, dcol};
    set_optional(ed.diag, h);
    return ed;
}

// Sparse quadratic objective: a KKT pass or report first forms g = c + Q x of the evaluated point -- one product with Q per pass,
// also for an average whose other products come out of the running sums -- and x'Qx with it; after the six sums are finished the
// objective's two slots go from g'x = c'x + x'Qx to the contract's c'x + 1/2 x'Qx and - 1/2 x'Qx (include/pdlp_hip.h).
template <typename T> int kkt_pass_begin(pdlp_handle h, int ix)
{
    if (!h->obj_mat.on) return PDLP_OK;
    h->carry.gradient_overwritten();       // (also at the current iterate: one rule for every pass)
    return obj_gradient<T, true>(h, ix);
}
inline int kkt_pass_end(pdlp_handle h, int gridA, int gridB)
{
    const int rc = finalize_kkt(h, gridA, gridB);
    return rc == PDLP_OK && h->obj_mat.on ? obj_matrix_finish(h) : rc;
}

template <typename T, bool UNSCALE, bool RANGED = false, bool QUAD = false> int kkt_local_u(pdlp_handle h, int which)
{
    const int ix = iterate_index(h, which);
    const T* dcol = UNSCALE ? (const T*)h->p.d_col : nullptr;
    const T* drow = UNSCALE ? (const T*)h->p.d_row : nullptr;
    int rc, gridA = grid_of(h->sKT, h->nl), gridB = grid_of(h->sK, h->ml);
    if ((rc = kkt_pass_begin<T>(h, ix)) != PDLP_OK) return rc;
    const bool kx_carried = which == PDLP_CUR && h->carry.kx_valid && !h->no_running;
    if (which == PDLP_AVG && h->carry.avg_products) {
        // K'y_avg (ktyb[1]) and K x_avg (kxb[2]) were formed from the running sums by pdlp_compute_average: two vector passes
        const auto ed = kkt_dual_epi<T, UNSCALE, QUAD>(h, ix, dcol, nullptr);
        if ((rc = epilogue_pass<T>(h, h->nl, h->ktyb[1], ed, h->partA)) != PDLP_OK) return rc;
        const auto ep = kkt_primal_epi<T, UNSCALE, RANGED>(h, ix, drow, nullptr);
        if ((rc = epilogue_pass<T>(h, h->ml, h->kxb[2], ep, h->partB)) != PDLP_OK) return rc;
        gridA = rows_grid(h->nl);
        gridB = rows_grid(h->ml);
    } else {
        T* kx_out = which == PDLP_CUR ? (T*)h->kxb[1] : (which == PDLP_AVG ? (T*)h->kxb[2] : nullptr);
        // K'y of a candidate is the product the first primal half-step after the check needs again (same kernel, same
        // sums): keep it.  (A pass at the current iterate after a restart to the average supersedes that restart's copy.)
        T* kty_out = which == PDLP_CUR ? (T*)h->ktyb[0] : (which == PDLP_AVG ? (T*)h->ktyb[1] : nullptr);
        h->carry.kkt_begins(which);
        const auto ed = kkt_dual_epi<T, UNSCALE, QUAD>(h, ix, dcol, kty_out);
        if ((rc = launch_csr<T>(h, true, h->yb[ix], ed, h->partA)) != PDLP_OK) return rc;
        if (kx_carried) {
            // K x of the current iterate is carried along by the dual half-steps (kxb[0]): no product
            const auto ep = kkt_primal_epi<T, UNSCALE, RANGED>(h, ix, drow, nullptr);
            if ((rc = epilogue_pass<T>(h, h->ml, h->kxb[0], ep, h->partB)) != PDLP_OK) return rc;
            gridB = rows_grid(h->ml);
        } else {
            const auto ep = kkt_primal_epi<T, UNSCALE, RANGED>(h, ix, drow, kx_out);
            if ((rc = launch_csr<T>(h, false, h->xb[ix], ep, h->partB)) != PDLP_OK) return rc;
        }
    }
    if ((rc = kkt_pass_end(h, gridA, gridB)) != PDLP_OK) return rc;
    h->carry.kkt_kept(which, kx_carried);
    return PDLP_OK;
}

template <typename T> int kkt_local_t(pdlp_handle h, int which, int unscaled)
{
    // (a handle may have two-sided rows and the quadratic term)
    return with_flags([&](auto U, auto R, auto Q) { return kkt_local_u<T, U.value, R.value, Q.value>(h, which); }, unscaled,
                      h->q_upper != nullptr, h->obj_diag != nullptr);
}

// Solution report (pdlp_report_local): reduced costs and row activities of an iterate stored, with the six KKT sums.  The two
// products are the plain ones of pdlp_spmv (StoreEpi: instantiated for every kernel family; float64 accumulation over the float32
// matrix in mixed precision, never the delta-mode anchors) written straight into the caller's vectors; a vector pass over each
// then forms the sums and turns K'y into lam in place.  A vector the caller does not want (null) costs nothing extra: that side
// runs the KKT pass's own fused epilogue without its stores.  Nothing of the solver's state is read except the iterate and
// nothing is written except scratch (partial sums, row sums, PDLP_BUF_RED).
template <typename T, bool UNSCALE, bool RANGED = false, bool QUAD = false> int report_local_u(pdlp_handle h, int which, void* rc_local, void* act_local)
{
    const int ix = iterate_index(h, which);
    const T* dcol = UNSCALE ? (const T*)h->p.d_col : nullptr;
    const T* drow = UNSCALE ? (const T*)h->p.d_row : nullptr;
    int rc, gridA = grid_of(h->sKT, h->nl), gridB = grid_of(h->sK, h->ml);
    if ((rc = kkt_pass_begin<T>(h, ix)) != PDLP_OK) return rc;
    if (rc_local) {
        StoreEpi<T> st{(T*)rc_local};
        if ((rc = launch_csr<T>(h, true, h->yb[ix], st, h->partA)) != PDLP_OK) return rc;
        const auto ed = report_dual_epi<T, UNSCALE, QUAD>(h, ix, dcol, (T*)rc_local);
        if ((rc = epilogue_pass<T>(h, h->nl, nullptr, ed, h->partA)) != PDLP_OK) return rc;
        gridA = rows_grid(h->nl);
    } else {
        const auto ed = kkt_dual_epi<T, UNSCALE, QUAD>(h, ix, dcol, nullptr);
        if ((rc = launch_csr<T>(h, true, h->yb[ix], ed, h->partA)) != PDLP_OK) return rc;
    }
    if (act_local) {
        StoreEpi<T> st{(T*)act_local};
        if ((rc = launch_csr<T>(h, false, h->xb[ix], st, h->partB)) != PDLP_OK) return rc;
        const auto ep = report_primal_epi<T, UNSCALE, RANGED>(h, ix, drow, (T*)act_local);
        if ((rc = epilogue_pass<T>(h, h->ml, nullptr, ep, h->partB)) != PDLP_OK) return rc;
        gridB = rows_grid(h->ml);
    } else {
        const auto ep = kkt_primal_epi<T, UNSCALE, RANGED>(h, ix, drow, nullptr);
        if ((rc = launch_csr<T>(h, false, h->xb[ix], ep, h->partB)) != PDLP_OK) return rc;
    }
    return kkt_pass_end(h, gridA, gridB);
}

template <typename T> int report_local_t(pdlp_handle h, int which, int unscaled, void* rc_local, void* act_local)
{
    return with_flags([&](auto U, auto R, auto Q) { return report_local_u<T, U.value, R.value, Q.value>(h, which, rc_local, act_local); },
                      unscaled, h->q_upper != nullptr, h->obj_diag != nullptr);
}

template <typename T> void kkt_finish_t(const double* r, double omega_d, double* out)
{
    // helpers.py:84-94,102-106 in the working precision
    const T p = (T)r[3], d = (T)r[5], lp = (T)r[1], un = (T)r[2];
    const T adj = d + lp + un;
    const T gap = adj - p;
    const T pr = (T)std::sqrt(r[4]), dr = (T)std::sqrt(r[0]);
    const T w = (T)omega_d, w2 = w * w;
    const T kkt = (T)std::sqrt((double)(w2 * (pr * pr) + (dr * dr) / w2 + gap * gap));
    out[0] = pr; out[1] = dr; out[2] = gap; out[3] = p; out[4] = adj; out[5] = kkt;
}

// the period's running product sums are being kept and are complete so far
inline bool sums_running(pdlp_handle h)
{
    return !h->delta && !h->carry.sums_broken && !h->no_running && !h->graph_ok && h->carry.since_reset > 0;
}

// a new averaging period (pdhg.py:58-60): x_sum, y_sum, eta_sum and the pending weight; `products`: the running product sums too
int zero_sums(pdlp_handle h, bool products)
{
    HIP_TRY(hipMemsetAsync(h->x_sum, 0, h->nl * h->es, h->stream));
    HIP_TRY(hipMemsetAsync(h->y_sum, 0, h->ml * h->es, h->stream));
    if (products) {
        HIP_TRY(hipMemsetAsync(h->kx_sum, 0, h->ml * h->es, h->stream));
        HIP_TRY(hipMemsetAsync(h->kty_sum, 0, h->nl * h->es, h->stream));
    }
    hipLaunchKernelGGL(k_reset_average, dim3(1), dim3(1), 0, h->stream, h->sc);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

template <typename T> int flush_t(pdlp_handle h, int adaptive)
{
    Carried& c = h->carry;
    const bool running = sums_running(h);
    if (adaptive) {
        // the weight of the current iterate became known only after its step-size rule: add it now
        hipLaunchKernelGGL(k_flush<T>, dim3(grid_for(h->nl)), dim3(BLOCK), 0, h->stream, h->nl, (T*)h->x_sum,
                           (const T*)xloc<T>(h, h->ix_cur), h->sc, (int)S_WPEND);
        hipLaunchKernelGGL(k_flush<T>, dim3(grid_for(h->ml)), dim3(BLOCK), 0, h->stream, h->ml, (T*)h->y_sum,
                           (const T*)yloc<T>(h, h->ix_cur), h->sc, (int)S_WPEND);
        if (running && c.kx_valid)
            hipLaunchKernelGGL(k_flush<T>, dim3(grid_for(h->ml)), dim3(BLOCK), 0, h->stream, h->ml, (T*)h->kx_sum, (const T*)h->kxb[0],
                               h->sc, (int)S_WPEND);
    }
    // K'y of the current y exists only if the KKT pass of the current iterate ran before this call (it keeps it in ktyb[0])
    if (running && !c.kty_tail_done) {
        if (c.cand_cur != CAND_NONE && c.kty_cur < 0) {
            hipLaunchKernelGGL(k_flush<T>, dim3(grid_for(h->nl)), dim3(BLOCK), 0, h->stream, h->nl, (T*)h->kty_sum, (const T*)h->ktyb[0],
                               h->sc, (int)(adaptive ? S_WPEND : S_ETA));
            c.flushed_tail();
        } else if (adaptive) {
            c.sums_end();                // the pending weight is cleared below: that term of the sum is lost until the next restart
        }
    }
    if (adaptive) hipLaunchKernelGGL(k_clear_pending, dim3(1), dim3(1), 0, h->stream, h->sc);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

template <typename T> int average_t(pdlp_handle h)
{
    hipLaunchKernelGGL(k_average<T>, dim3(grid_for(h->nl)), dim3(BLOCK), 0, h->stream, h->nl, xloc<T>(h, h->ix_avg),
                       (const T*)h->x_sum, h->sc);
    hipLaunchKernelGGL(k_average<T>, dim3(grid_for(h->ml)), dim3(BLOCK), 0, h->stream, h->ml, yloc<T>(h, h->ix_avg),
                       (const T*)h->y_sum, h->sc);
    // the products of the average from the running sums (K is linear): K x_avg = sum w_k K x_k / sum w_k, the same for K'y
    const bool from_sums = sums_running(h) && h->carry.kty_tail_done && h->carry.kx_valid;
    if (from_sums) {
        hipLaunchKernelGGL(k_average<T>, dim3(grid_for(h->ml)), dim3(BLOCK), 0, h->stream, h->ml, (T*)h->kxb[2], (const T*)h->kx_sum, h->sc);
        hipLaunchKernelGGL(k_average<T>, dim3(grid_for(h->nl)), dim3(BLOCK), 0, h->stream, h->nl, (T*)h->ktyb[1], (const T*)h->kty_sum, h->sc);
    }
    h->carry.averaged(from_sums);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

template <typename T> int distance_t(pdlp_handle h)
{
    const int ga = grid_for(h->nl), gb = grid_for(h->ml);
    hipLaunchKernelGGL(k_sqdiff<T>, dim3(ga), dim3(BLOCK), 0, h->stream, h->nl, (const T*)h->x_last,
                       (const T*)xloc<T>(h, h->ix_cur), h->partA);
    hipLaunchKernelGGL(k_sqdiff<T>, dim3(gb), dim3(BLOCK), 0, h->stream, h->ml, (const T*)h->y_last,
                       (const T*)yloc<T>(h, h->ix_cur), h->partB);
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, h->stream, h->partA, ga, 1, h->red, 0);
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, h->stream, h->partB, gb, 1, h->red, 1);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// dx, dy of the step just taken (cur vs prev) into this rank's blocks of the full-length buffers
template <typename T> int infeas_begin_t(pdlp_handle h)
{
    if (h->nl > 0)
        hipLaunchKernelGGL(k_sub<T>, dim3(grid_for(h->nl)), dim3(BLOCK), 0, h->stream, h->nl, (T*)h->dxf + h->p.col0,
                           (const T*)xloc<T>(h, h->ix_cur), (const T*)xloc<T>(h, h->ix_prev));
    if (h->ml > 0)
        hipLaunchKernelGGL(k_sub<T>, dim3(grid_for(h->ml)), dim3(BLOCK), 0, h->stream, h->ml, (T*)h->dyf + h->p.row0,
                           (const T*)yloc<T>(h, h->ix_cur), (const T*)yloc<T>(h, h->ix_prev));
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// three products (K'dy, K'y with the variable-side tests fused, K dx with the constraint-side tests fused) and the
// eight partial sums of detect_infeasibility into red[0..7]
template <typename T> int infeas_local_t(pdlp_handle h, double tol)
{
    int rc;
    if ((rc = spmv_t<T>(h, 1, h->dyf, h->ktdy)) != PDLP_OK) return rc;
    InfeasDualEpi<T> ed{xloc<T>(h, h->ix_cur), xloc<T>(h, h->ix_prev), (const T*)h->p.c, (const T*)h->p.l, (const T*)h->p.u,
                        (const T*)h->ktdy, (T*)h->lam_prev, (T)tol};
    if ((rc = launch_csr<T>(h, true, h->yb[h->ix_cur], ed, h->partA)) != PDLP_OK) return rc;
    InfeasPrimalEpi<T> ep{yloc<T>(h, h->ix_cur), yloc<T>(h, h->ix_prev), (const T*)h->p.q, (T)tol, h->ineq_end};
    if ((rc = launch_csr<T>(h, false, h->dxf, ep, h->partB)) != PDLP_OK) return rc;
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, h->stream, h->partA, grid_of(h->sKT, h->nl), 4, h->red, 0);
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, h->stream, h->partB, grid_of(h->sK, h->ml), 4, h->red, 4);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// the decisions of enhancements.py:118-142 and :148-159 from the eight sums, in the working precision
template <typename T> int infeas_decide_t(const double* r, double tol, double* diag)
{
    const T t = (T)tol;
    const T dres = (T)std::sqrt(r[0]), lu = (T)r[1], cdx = (T)r[2], eqn = (T)std::sqrt(r[4]), qdy = (T)r[7];
    diag[0] = eqn; diag[1] = r[5]; diag[2] = cdx; diag[3] = r[3]; diag[4] = dres; diag[5] = r[6]; diag[6] = qdy; diag[7] = lu;
    if (eqn < t && r[5] == 0.0 && cdx < t && r[3] == 0.0) return 1;                      // "DUAL_INFEASIBLE"
    if (dres < t && r[6] == 0.0 && (double)qdy - (double)lu > -tol) return 2;            // "PRIMAL_INFEASIBLE"
    return 0;
}

template <typename T> int power_iteration_t(pdlp_handle h, const void* b0, int iters, void* work_n, void* work_m, double* sigma)
{
    T* b = (T*)work_n;
    T* t = (T*)work_m;
    int rc;
    HIP_TRY(hipMemcpyAsync(b, b0, (size_t)h->p.n * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
    const int g = grid_for(h->p.n);
    for (int it = 0; it < iters; ++it) {                                   // helpers.py:48-50
        if ((rc = spmv_t<T>(h, 0, b, t)) != PDLP_OK) return rc;
        if ((rc = spmv_t<T>(h, 1, t, b)) != PDLP_OK) return rc;
        hipLaunchKernelGGL(k_sqdiff<T>, dim3(g), dim3(BLOCK), 0, h->stream, h->p.n, (const T*)b, (const T*)nullptr, h->partA);
        hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, h->stream, h->partA, g, 1, h->red, 0);
        hipLaunchKernelGGL(k_div_by_norm<T>, dim3(g), dim3(BLOCK), 0, h->stream, h->p.n, b, h->red, 0);
    }
    if ((rc = spmv_t<T>(h, 0, b, t)) != PDLP_OK) return rc;               // helpers.py:51
    const int gm = grid_for(h->p.m);
    hipLaunchKernelGGL(k_sqdiff<T>, dim3(gm), dim3(BLOCK), 0, h->stream, h->p.m, (const T*)t, (const T*)nullptr, h->partA);
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, h->stream, h->partA, gm, 1, h->red, 0);
    HIP_TRY(hipGetLastError());
    double r = 0.0;
    HIP_TRY(hipMemcpyAsync(&r, h->red, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *sigma = (double)(T)std::sqrt(r);
    return PDLP_OK;
}

}  // namespace

extern "C" {

int pdlp_restart(pdlp_handle h, int which)
{
    if (!h || (which != PDLP_CUR && which != PDLP_AVG)) return PDLP_ERR_INVALID;
    const int cand = which == PDLP_CUR ? 0 : 1;
    h->carry.buffers_reassigned();      // (t = 0 again: the next fixed-point residual belongs to the next Halpern iteration)
    if (which == PDLP_AVG) {       // the averaged iterate becomes current (pdhg.py:133,137,141)
        const int t = h->ix_cur;
        h->ix_cur = h->ix_avg;
        h->ix_avg = t;
    }
    // K x and K'y of the chosen point as its KKT pass left them follow the iterate: the K x cache unless the pass read it from there;
    // delta mode: the average's pair becomes the anchors (the current iterate's anchors are in place)
    if (cand == 1 ? h->carry.cand_avg : h->carry.cand_cur == CAND_KX_OWN) {
        char* t = h->kxb[0]; h->kxb[0] = h->kxb[1 + cand]; h->kxb[1 + cand] = t;
        if (h->delta) { t = h->ktyr; h->ktyr = h->ktyb[1]; h->ktyb[1] = t; }
    }
    h->carry.restart_adopted(cand, h->delta);
    return zero_sums(h, !h->delta);
}

}  // extern "C"
