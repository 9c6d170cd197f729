// pdlp_halpern.inc -- the restarted, reflected Halpern iteration (pdlp_halpern_iterate, include/pdlp_hip.h): two fused products
// per iteration like the PDHG step, with HalpernPrimalEpi / HalpernDualEpi as their epilogues.  The iterate z lives in the PDLP_CUR
// buffers, the candidate T(z) -- one fixed PDHG step from z -- in the PDLP_AVG buffers, the anchor is the restart point (x_last,
// y_last) and t is the handle's count of iterations since the last restart.  The old z stays behind in the PDLP_PREV buffers, so the
// fixed-point residual z - T(z) of the last iteration (pdlp_halpern_fixed_point) is one vector pass and one product.  The reference
// has no counterpart.
// Part of pdlp_hip.hip (included at file scope; not a translation unit of its own).  Needs: pdlp_products.inc and what is before it.
// ------------------------------------------------------------------------------------------------
namespace {

template <typename T, bool RANGED, bool QUAD> int halpern_iterate_e(pdlp_handle h, int iters)
{
    int rc;
    for (int it = 0; it < iters; ++it) {
        // a = (t+1)/(t+2), b = 1/(t+2) in double, rounded once to the working type
        const double t2 = (double)(h->carry.since_reset + 2);
        const T a = (T)((double)(h->carry.since_reset + 1) / t2), b = (T)(1.0 / t2);
        const int cur = h->ix_cur, nxt = h->ix_prev, cand = h->ix_avg;
        // QUAD: diagonal quadratic objective (pdlp_set_objective_diag); RANGED: two-sided rows (pdlp_set_row_upper)
        HalpernPrimalEpi<T, QUAD> ep{xloc<T>(h, cur), xloc<T>(h, nxt), (T*)h->xbar + h->p.col0, xloc<T>(h, cand), (const T*)h->x_last,
                                     (const T*)h->p.c, (const T*)h->p.l, (const T*)h->p.u, h->sc, a, b};
        set_optional(ep.diag, h);
        if ((rc = launch_csr<T>(h, true, h->yb[cur], ep, h->partA)) != PDLP_OK) return rc;
        HalpernDualEpi<T, RANGED> ed{yloc<T>(h, cur), yloc<T>(h, nxt), yloc<T>(h, cand), (const T*)h->y_last, (const T*)h->p.q, h->sc,
                                     h->ineq_end, a, b};
        set_optional(ed.upper, h);
        if ((rc = launch_csr<T>(h, false, h->xbar, ed, h->partB)) != PDLP_OK) return rc;
        h->ix_cur = nxt;           // the freshly written z becomes current; the old z's buffers are the next iteration's target
        h->ix_prev = cur;
        h->carry.halpern_iterated();
    }
    return PDLP_OK;
}

template <typename T> int halpern_iterate_t(pdlp_handle h, int iters)
{
    return with_flags([&](auto R, auto Q) { return halpern_iterate_e<T, R.value, Q.value>(h, iters); }, h->q_upper != nullptr,
                      h->obj_diag != nullptr);
}

// The fixed-point residual of the last iteration: z = PDLP_PREV, T(z) = PDLP_AVG.  One vector pass (dy into the detector's full-length
// buffer, which this mode never uses otherwise, with ||dy||^2), one product K'dy with FixedPointEpi, two finishes.
template <typename T> int halpern_fixed_point_t(pdlp_handle h)
{
    const int prev = h->ix_prev, cand = h->ix_avg;
    const int gb = grid_for(h->ml);
    hipLaunchKernelGGL(k_sub_sq<T>, dim3(gb), dim3(BLOCK), 0, h->stream, h->ml, (T*)h->dyf + h->p.row0, (const T*)yloc<T>(h, prev),
                       (const T*)yloc<T>(h, cand), h->partB);
    FixedPointEpi<T> ep{xloc<T>(h, prev), xloc<T>(h, cand)};
    int rc;
    if ((rc = launch_csr<T>(h, true, h->dyf, ep, h->partA)) != PDLP_OK) return rc;
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, h->stream, h->partA, grid_of(h->sKT, h->nl), 2, h->red, 0);
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, h->stream, h->partB, gb, 1, h->red, 2);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// the forms the Halpern mode does not have: mixed precision / delta mode, a shard of a problem, an exchange of any kind, graph replay,
// and a sparse quadratic objective (the reflected operator 2T - I of the linearised step is not non-expansive)
inline bool halpern_refused(pdlp_handle h)
{
    return !plain_single(h) || h->graph_ok || h->obj_mat.on;
}

}  // namespace

extern "C" {

int pdlp_halpern_iterate(pdlp_handle h, int iters)
{
    if (!h || iters < 0) return PDLP_ERR_INVALID;
    if (halpern_refused(h)) return PDLP_ERR_STATE;
    if (iters == 0) return PDLP_OK;
    char rname[64];
    if (g_roctx.level > 0) std::snprintf(rname, sizeof rname, "pdlp: %d Halpern iterations", iters);
    Range range(rname, h->stream);
    h->carry.halpern_begins();     // nothing carried from before survives; PDLP_AVG holds the candidate from now on
    return DISPATCH(h, halpern_iterate_t, h, iters);
}

int pdlp_halpern_fixed_point(pdlp_handle h)
{
    if (!h) return PDLP_ERR_INVALID;
    if (halpern_refused(h) || !h->carry.halpern_pair) return PDLP_ERR_STATE;
    Range range("pdlp: Halpern fixed-point residual", h->stream);
    return DISPATCH(h, halpern_fixed_point_t, h);
}

}  // extern "C"
