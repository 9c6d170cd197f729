// pdlp_delta.inc -- delta mode (mixed precision): every product of the iteration runs on the float32 kernels over a float32
// DIFFERENCE vector and is added to a float64 anchor product that is carried along (pdlp_solver::delta; Carried: anchors_valid,
// dy_folded).  The exact anchors (delta_refresh), the two half-steps, the KKT sums of a candidate from the anchors, and the entry
// points that switch the mode and set or report the anchors' state.
// Part of pdlp_hip.hip (included at file scope; not a translation unit of its own).  Needs: pdlp_products.inc and what is before it.
// ------------------------------------------------------------------------------------------------
namespace {

// exact anchors: KX = K x_cur and KTY = K'y_cur by the mixed-precision kernels (float64 gathers, products and sums)
int delta_refresh(pdlp_handle h)
{
    int rc;
    StoreEpi<double> ex{(double*)h->kxb[0]};
    if ((rc = launch_mat<double, float, StoreEpi<double>>(h, false, h->xb[h->ix_cur], ex, h->partB)) != PDLP_OK) return rc;
    StoreEpi<double> ey{(double*)h->ktyr};
    if ((rc = launch_mat<double, float, StoreEpi<double>>(h, true, h->yb[h->ix_cur], ey, h->partA)) != PDLP_OK) return rc;
    h->carry.anchors_exact();
    return PDLP_OK;
}

template <bool ADAPT, bool PEER> int delta_primal_half_a(pdlp_handle h)
{
    int rc;
    if (!h->carry.anchors_valid && (rc = delta_refresh(h)) != PDLP_OK) return rc;
    DeltaPrimalEpi<ADAPT, PEER> e{(const double*)xloc<double>(h, h->ix_cur), xloc<double>(h, h->ix_prev), h->gdx + h->p.col0, (const double*)h->p.c,
                                  (const double*)h->p.l, (const double*)h->p.u, (double*)h->x_sum, (double*)h->ktyr, h->sc};
    peer_targets(h, e.peer, 4);
    if (h->carry.dy_folded && !h->sKT.pending) {
        // K'y of the current y is already in the anchor (a restart check folded dy in, or the anchors are fresh): vector pass
        if (h->range_sel > 0) return PDLP_OK;                // (issued piece by piece: all of it went out with piece 0)
        h->last_gridA = rows_grid(h->nl);
        return epilogue_pass<float>(h, h->nl, nullptr, e, h->partA);
    }
    const PieceCtl pc = piece_ctl(h, h->sKT);
    if (pc.skip) return PDLP_OK;
    h->last_gridA = grid_of(h->sKT, h->nl);
    h->use_split = true;
    rc = launch_mat<float, float, DeltaPrimalEpi<ADAPT, PEER>>(h, true, h->gdy, e, h->partA);
    h->use_split = false;
    if (pc.finish || rc != PDLP_OK) {
        h->sKT.pending = false;
        h->carry.folded();
    }
    return rc;
}

template <bool ADAPT, bool PEER> int delta_dual_half_a(pdlp_handle h)
{
    DeltaDualEpi<ADAPT, PEER> e{(const double*)yloc<double>(h, h->ix_cur), yloc<double>(h, h->ix_prev), h->gdy + h->p.row0, (const double*)h->p.q,
                                (double*)h->y_sum, (double*)h->kxb[0], h->sc, h->ineq_end};
    peer_targets(h, e.peer, 5);
    const PieceCtl pc = piece_ctl(h, h->sK);
    int rc = PDLP_OK;
    if (!pc.skip) {
        h->last_gridB = grid_of(h->sK, h->ml);
        h->use_split = true;
        rc = launch_mat<float, float, DeltaDualEpi<ADAPT, PEER>>(h, false, h->gdx, e, h->partB);
        h->use_split = false;
    }
    if (rc != PDLP_OK) { h->sK.pending = false; return rc; }
    if (!pc.finish) return PDLP_OK;
    h->sK.pending = false;
    const int t = h->ix_cur;
    h->ix_cur = h->ix_prev;
    h->ix_prev = t;
    h->carry.iterated(1, true);
    return PDLP_OK;
}

int delta_primal_half(pdlp_handle h, int adaptive)
{
    return with_flags([&](auto A, auto P) { return delta_primal_half_a<A.value, P.value>(h); }, adaptive, h->peer.active);
}
int delta_dual_half(pdlp_handle h, int adaptive)
{
    return with_flags([&](auto A, auto P) { return delta_dual_half_a<A.value, P.value>(h); }, adaptive, h->peer.active);
}

// KKT sums of a candidate from the anchors: the current iterate needs at most the pending K'dy; the averaged / previous
// iterate two float32 products over float32(candidate - current) added to the anchors
// the current iterate's KKT sums from the anchors; UNSCALE: of the un-preconditioned problem (pdhg.py:157-161)
template <bool UNSCALE> int delta_kkt_cur(pdlp_handle h)
{
    int rc, gridA = rows_grid(h->nl);
    typedef KktDualEpi<double, UNSCALE> KD;
    typedef KktPrimalEpi<double, UNSCALE> KP;
    KD ed{xloc<double>(h, h->ix_cur), (const double*)h->p.c, (const double*)h->p.l, (const double*)h->p.u,
          UNSCALE ? (const double*)h->p.d_col : nullptr, nullptr};
    if (!h->carry.dy_folded) {
        AnchorEpi<KD, true> e{ed, (double*)h->ktyr};
        if ((rc = launch_mat<float, float, AnchorEpi<KD, true>>(h, true, h->gdy, e, h->partA)) != PDLP_OK) return rc;
        h->carry.folded();
        gridA = grid_of(h->sKT, h->nl);
    } else {
        if ((rc = epilogue_pass<double>(h, h->nl, h->ktyr, ed, h->partA)) != PDLP_OK) return rc;
    }
    KP ep{yloc<double>(h, h->ix_cur), (const double*)h->p.q, UNSCALE ? (const double*)h->p.d_row : nullptr, nullptr, h->ineq_end};
    if ((rc = epilogue_pass<double>(h, h->ml, h->kxb[0], ep, h->partB)) != PDLP_OK) return rc;
    if ((rc = finalize_kkt(h, gridA, rows_grid(h->ml))) != PDLP_OK) return rc;
    h->carry.kkt_kept(PDLP_CUR, true);
    return PDLP_OK;
}

int delta_kkt_local(pdlp_handle h, int which, int unscaled)
{
    int rc;
    if (!h->carry.anchors_valid && (rc = delta_refresh(h)) != PDLP_OK) return rc;
    typedef KktDualEpi<double, false> KD;
    typedef KktPrimalEpi<double, false> KP;
    if (which == PDLP_CUR) return unscaled ? delta_kkt_cur<true>(h) : delta_kkt_cur<false>(h);
    if (unscaled) return PDLP_ERR_STATE;                  // (the driver evaluates the un-scaled problem at the current iterate only)
    if (!h->carry.dy_folded) {
        FoldEpi f{(double*)h->ktyr};
        if ((rc = launch_mat<float, float, FoldEpi>(h, true, h->gdy, f, h->partA)) != PDLP_OK) return rc;
        h->carry.folded();
    }
    const int ix = which == PDLP_AVG ? h->ix_avg : h->ix_prev;
    // the full-length differences (every rank holds the complete candidate and the complete current iterate)
    hipLaunchKernelGGL(k_diff_f32, dim3(grid_for(h->p.n)), dim3(BLOCK), 0, h->stream, h->p.n, h->gdx, (const double*)h->xb[ix],
                       (const double*)h->xb[h->ix_cur]);
    hipLaunchKernelGGL(k_diff_f32, dim3(grid_for(h->p.m)), dim3(BLOCK), 0, h->stream, h->p.m, h->gdy, (const double*)h->yb[ix],
                       (const double*)h->yb[h->ix_cur]);
    // K'y and K x of the averaged iterate are kept: a restart to it adopts them as the new anchors
    KD ed{xloc<double>(h, ix), (const double*)h->p.c, (const double*)h->p.l, (const double*)h->p.u, nullptr,
          which == PDLP_AVG ? (double*)h->ktyb[1] : nullptr};
    AnchorEpi<KD, false> ea{ed, (double*)h->ktyr};
    if ((rc = launch_mat<float, float, AnchorEpi<KD, false>>(h, true, h->gdy, ea, h->partA)) != PDLP_OK) return rc;
    KP ep{yloc<double>(h, ix), (const double*)h->p.q, nullptr, which == PDLP_AVG ? (double*)h->kxb[2] : nullptr, h->ineq_end};
    AnchorEpi<KP, false> eb{ep, (double*)h->kxb[0]};
    if ((rc = launch_mat<float, float, AnchorEpi<KP, false>>(h, false, h->gdx, eb, h->partB)) != PDLP_OK) return rc;
    if ((rc = finalize_kkt(h, grid_of(h->sKT, h->nl), grid_of(h->sK, h->ml))) != PDLP_OK) return rc;
    h->carry.kkt_kept(which, false);
    return PDLP_OK;
}

}  // namespace

extern "C" {

int pdlp_set_delta(pdlp_handle h, int on)
{
    if (!h) return PDLP_ERR_INVALID;
    if (on && (!h->mixed || h->q_upper)) return PDLP_ERR_STATE;           // float32 matrix values under float64 vectors only, one-sided rows
    if ((on != 0) == h->delta) return PDLP_OK;
    drop_graphs(h);
    h->graph_ok = false;
    h->delta = on != 0;
    h->carry.drop_products();
    return PDLP_OK;
}

int pdlp_set_anchors(pdlp_handle h, const void* kx_local, const void* kty_local)
{
    if (!h || !kx_local || !kty_local) return PDLP_ERR_INVALID;
    if (!h->delta) return PDLP_ERR_STATE;
    HIP_TRY(hipMemcpyAsync(h->kxb[0], kx_local, (size_t)h->ml * 8, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->ktyr, kty_local, (size_t)h->nl * 8, hipMemcpyDeviceToDevice, h->stream));
    h->carry.anchors_given();
    return PDLP_OK;
}

int pdlp_delta_state(pdlp_handle h, int32_t out[3])
{
    if (!h || !out) return PDLP_ERR_INVALID;
    out[0] = h->delta; out[1] = h->carry.anchors_valid; out[2] = h->carry.dy_folded;
    return PDLP_OK;
}

}  // extern "C"
