// pdlp_products.inc -- the products and the half-steps.  launch_mat: one product with K or K' with a fused epilogue, in every form
// (CSR row blocks, tiles in one launch, tiles in panel groups, a split product's phases and output pieces); launch_csr picks the
// matrix type of the handle's precision.  Then the launches every later file shares (epilogue_pass, finalize_kkt, iterate_index,
// launch_adaptive_rule, with_flags), the primal and dual half-steps, their early parts for sharded problems (half_begin_t,
// half_chunk_t, half_piece) and the plain product (spmv_t).  The objective's matrix Q (pdlp_set_objective_matrix) has its own
// launcher over the CSR form alone (launch_obj_matrix) and the gradient product ahead of every primal half-step (obj_gradient).
// Part of pdlp_hip.hip (included at file scope; not a translation unit of its own).  Needs: pdlp_schedule.inc and what is before it.
// ------------------------------------------------------------------------------------------------
namespace {

// partial row sums of `vgroups` panel groups over `vtotal` panels in virtual order (see k_tiled_fused) into
// rowsum[slot0 .. slot0 + vgroups); the epilogue functor is not used by these launches
template <typename T, typename TV>
void launch_tiled_groups(pdlp_handle h, const Schedule& s, int rows, const void* vin, hipStream_t stream, int vgroups, int vtotal,
                         const int32_t* ptab, int slot0, int b0 = 0, int nbl = -1)
{
    if (nbl < 0) nbl = s.t.nblk - b0;                     // (default: every row block)
    if (vtotal <= 0 || vgroups <= 0 || nbl <= 0) return;
    const int groups = vgroups < vtotal ? vgroups : vtotal;       // (the kernel splits the panels evenly: no group without panels)
    StoreEpi<T> none{nullptr};
    if constexpr (std::is_same<T, float>::value && std::is_same<TV, float>::value) {
        if (s.idx24) {      // the packed index stream (pdlp_attach_packed_items): same sums from 7 bytes per item
            hipLaunchKernelGGL((k_tiled_fused<T, TV, StoreEpi<T>, false, true>), dim3(nbl * groups), dim3(TNT), 0, stream, s.idx24,
                               (const TV*)s.t.val, s.t.tile_ptr, s.t.blk_base, s.t.cnt, s.run_base, s.t.npanel, s.t.lw, s.t.rpt, rows, s.t.nblk,
                               vtotal, ptab, slot0, b0, nbl, (const T*)vin, (T*)h->rowsum, h->rs_stride, (const T*)nullptr, none, (double*)nullptr);
            return;
        }
    }
    hipLaunchKernelGGL((k_tiled_fused<T, TV, StoreEpi<T>, false>), dim3(nbl * groups), dim3(TNT), 0, stream, s.t.idx,
                       (const TV*)s.t.val, s.t.tile_ptr, s.t.blk_base, s.t.cnt, (const uint32_t*)nullptr, s.t.npanel, s.t.lw, s.t.rpt, rows,
                       s.t.nblk, vtotal, ptab, slot0, b0, nbl, (const T*)vin, (T*)h->rowsum, h->rs_stride, (const T*)nullptr, none,
                       (double*)nullptr);
}

// one phase of a split product (0: the own block's panels, 1 + c: the panels completed by chunk c of the exchange), over all row
// blocks or over the row blocks [b0, b0 + nbl) of one output piece (the last phase of a product whose result travels in pieces)
template <typename T, typename TV>
void launch_phase(pdlp_handle h, const Schedule& s, int rows, const void* vin, hipStream_t stream, int phase, int b0 = 0, int nbl = -1)
{
    launch_tiled_groups<T, TV>(h, s, rows, vin, stream, s.ph_slots[phase], s.ph_cnt[phase], s.ptab + s.ph_off[phase], s.ph_slot0[phase], b0, nbl);
}

// the CSR form of a product: the row blocks of schedule `s` over the arrays (ci, va) -- K's, K''s or Q's -- and the epilogue of the
// rows that were multiplied in chunks; partial sums of s.grid (+ s.lgrid) workgroups
template <typename T, typename TV, class Epi, bool SORTED>
void launch_csr_rows(pdlp_handle h, const Schedule& s, const int32_t* ci, const TV* va, const void* vin, Epi epi, double* partials)
{
    // (s.rplo, the low words of the row pointers: csr_pass needs block-relative offsets only)
    hipLaunchKernelGGL((k_csr_fused<T, TV, Epi, SORTED>), dim3(s.grid), dim3(BLOCK), 0, h->stream, s.blk, s.nblk, s.lch, s.nchunks,
                       (T*)s.longpart, s.rplo, ci, va, SORTED ? s.sidx : (const uint32_t*)nullptr, SORTED ? (const TV*)s.sval : (const TV*)nullptr,
                       SORTED ? s.cbase : (const int32_t*)nullptr, (const T*)vin, epi, partials);
    if (s.nlong > 0)
        hipLaunchKernelGGL((k_long_rows<T, Epi>), dim3(s.lgrid), dim3(BLOCK), 0, h->stream, s.lrow, s.lptr, s.nlong,
                           (const T*)s.longpart, epi, partials + (size_t)s.grid * NACC);
}

// one product with K (or K') over the vector vin with the epilogue fused: T = type of vin, of the row sums and of what the
// epilogue receives, TV = type of the stored matrix values
template <typename T, typename TV, class Epi>
int launch_mat(pdlp_handle h, bool transpose, const void* vin, Epi epi, double* partials)
{
    if (!h->use_split && (h->sK.pending || h->sKT.pending)) {
        // an early local-panel product that nobody is going to consume (the caller changed course): let it finish
        // before the row-sum scratch is reused
        if (!(h->sK.pending ? h->sK.pending_inline : h->sKT.pending_inline)) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_out, 0));
        h->sK.pending = h->sKT.pending = false;
        h->sK.chunks_done = h->sKT.chunks_done = 0;
    }
    const Schedule& s = transpose ? h->sKT : h->sK;
    if (s.nblk == 0) return PDLP_OK;
    if (s.tiled) {
        const int rows = (int)(transpose ? h->nl : h->ml);
        // the remainder (items the tile format could not hold) first: its row sums go to a dense vector the epilogue adds
        const T* extra = nullptr;
        if (s.t.rem_rows_n > 0 && h->range_sel > 0) {
            extra = (const T*)(sizeof(T) == 4 && h->es == 8 ? s.t.rem_extra_f32 : s.t.rem_extra);     // (computed with piece 0 of this half-step)
        } else if (s.t.rem_rows_n > 0) {
            T* ex = (T*)(sizeof(T) == 4 && h->es == 8 ? s.t.rem_extra_f32 : s.t.rem_extra);
            hipLaunchKernelGGL((k_rem_segments<T, TV>), dim3(grid_for((int64_t)s.t.rem_segs_n * 8)), dim3(BLOCK), 0, h->stream, s.t.rem_segs_n,
                               s.t.rem_sptr, s.t.rem_col, (const TV*)s.t.rem_val, (const T*)vin, (T*)s.t.rem_work);
            hipLaunchKernelGGL((k_rem_rows<T>), dim3(grid_for((int64_t)s.t.rem_rows_n * 8)), dim3(BLOCK), 0, h->stream, s.t.rem_rows_n, s.t.rem_rows,
                               s.t.rem_rptr, (const T*)s.t.rem_work, ex);
            extra = ex;
        }
        if (s.t.groups == 1 && !(s.pending && h->use_split)) {
            bool packed = false;
            if constexpr (std::is_same<T, float>::value && std::is_same<TV, float>::value) {
                if ((packed = s.idx24 != nullptr))
                    hipLaunchKernelGGL((k_tiled_fused<T, TV, Epi, true, true>), dim3(s.t.nblk), dim3(TNT), 0, h->stream, s.idx24, (const TV*)s.t.val,
                                       s.t.tile_ptr, s.t.blk_base, s.t.cnt, s.run_base, s.t.npanel, s.t.lw, s.t.rpt, rows, s.t.nblk, s.t.npanel,
                                       (const int32_t*)nullptr, 0, 0, s.t.nblk, (const T*)vin, (T*)h->rowsum, h->rs_stride, extra, epi, partials);
            }
            if (!packed)
                hipLaunchKernelGGL((k_tiled_fused<T, TV, Epi, true>), dim3(s.t.nblk), dim3(TNT), 0, h->stream, s.t.idx, (const TV*)s.t.val,
                                   s.t.tile_ptr, s.t.blk_base, s.t.cnt, (const uint32_t*)nullptr, s.t.npanel, s.t.lw, s.t.rpt, rows, s.t.nblk,
                                   s.t.npanel, (const int32_t*)nullptr, 0, 0, s.t.nblk, (const T*)vin, (T*)h->rowsum, h->rs_stride, extra, epi,
                                   partials);
        } else if (s.pending && h->use_split) {
            // the local panels were multiplied by pdlp_*_half_begin on the side stream (and the first chunks' panels by
            // pdlp_half_chunk as they arrived); now the remaining chunks' panels, then the sum over all slots in fixed order.
            // If the RESULT travels in pieces (nrange > 1: the next exchange is chunked), the last phase and the epilogue run piece
            // by piece -- the row blocks of piece 0, its epilogue, an event; then piece 1 ... -- so that a piece's collective can
            // start while the rows of the later pieces are still being multiplied.  h->range_sel >= 0: only that piece (the caller
            // issues the piece's collective after every call), else all of them.
            Schedule& sm = transpose ? h->sKT : h->sK;
            const int R = s.nrange > 1 ? s.nrange : 1, last = s.nphase - 1;
            const int r_from = h->range_sel < 0 ? 0 : h->range_sel, r_to = h->range_sel < 0 ? R : h->range_sel + 1;
            if (r_from == 0) {
                for (int ph = 1 + sm.chunks_done; ph < (R > 1 ? last : s.nphase); ++ph) launch_phase<T, TV>(h, s, rows, vin, h->stream, ph);
                sm.chunks_done = 0;
            }
            int pofs = 0;
            for (int r = 0; r < r_from && R > 1; ++r) pofs += range_epi_grid(s, r, rows);
            for (int r = r_from; r < r_to && r < R; ++r) {
                if (R > 1) launch_phase<T, TV>(h, s, rows, vin, h->stream, last, s.rb_lo[r], s.rb_lo[r + 1] - s.rb_lo[r]);
                if (r == 0 && !s.pending_inline) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_out, 0));
                const int lo = R > 1 ? range_rows_lo(s, r) : 0, hi = R > 1 ? range_rows_hi(s, r, rows) : rows;
                if (hi > lo)
                    hipLaunchKernelGGL((k_rowsum_epilogue<T, Epi>), dim3(grid_for(hi - lo)), dim3(BLOCK), 0, h->stream, (const T*)h->rowsum,
                                       s.slotsA + s.slotsB, h->rs_stride, hi, extra, epi, partials + (size_t)pofs * NACC, lo);
                pofs += R > 1 ? range_epi_grid(s, r, rows) : 0;
            }
        } else {
            launch_tiled_groups<T, TV>(h, s, rows, vin, h->stream, s.t.groups, s.t.npanel, (const int32_t*)nullptr, 0);
            hipLaunchKernelGGL((k_rowsum_epilogue<T, Epi>), dim3(grid_for(rows)), dim3(BLOCK), 0, h->stream, (const T*)h->rowsum,
                               s.t.groups, h->rs_stride, rows, extra, epi, partials);
        }
        HIP_TRY(hipGetLastError());
        return PDLP_OK;
    }
    const int32_t* ci = transpose ? h->p.KT_colidx : h->p.K_colidx;
    const TV* va = (const TV*)(transpose ? h->p.KT_val : h->p.K_val);
    if (s.sidx) launch_csr_rows<T, TV, Epi, true>(h, s, ci, va, vin, epi, partials);
    else launch_csr_rows<T, TV, Epi, false>(h, s, ci, va, vin, epi, partials);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// A functor in its RANGED or QUAD form exists only over a matrix in the working type -- a handle with two-sided rows or a quadratic
// objective is one GPU in one precision (pdlp_set_row_upper, pdlp_set_objective_diag) -- and says so itself (working_matrix_only
// beside its optional operand, pdlp_epilogues.inc): no float32-matrix product is built for it.
template <class Epi, class = void> struct working_matrix_only : std::false_type {};
template <class Epi> struct working_matrix_only<Epi, std::void_t<decltype(Epi::working_matrix_only)>> : std::bool_constant<Epi::working_matrix_only> {};

// the product in the handle's working precision T (the matrix is float32 under float64 vectors in mixed precision): the one place
// that chooses the matrix type
template <typename T, class Epi>
int launch_csr(pdlp_handle h, bool transpose, const void* vin, Epi epi, double* partials)
{
    if constexpr (std::is_same<T, double>::value && !working_matrix_only<Epi>::value) {
        if (h->mixed) return launch_mat<double, float, Epi>(h, transpose, vin, epi, partials);
    }
    return launch_mat<T, T, Epi>(h, transpose, vin, epi, partials);
}

inline int grid_of(const Schedule& s, int64_t rows)
{
    if (s.nblk == 0) return 0;
    if (!s.tiled) return s.grid + (s.nlong > 0 ? s.lgrid : 0);
    if (s.t.groups == 1 && !s.pending) return s.t.nblk;
    return s.pending ? split_epi_grid(s, (int)rows) : grid_for(rows);      // split tiles: the partial sums come from k_rowsum_epilogue
}

// A half-step issued piece by piece (pdlp_*_half_piece: h->range_sel = the piece, h->range_cnt = their number).  Only a split product
// whose result travels in pieces really runs piece by piece (launch_mat); every other form of the half-step does all its work with
// piece 0 and nothing afterwards.  The state changes that end a half-step (buffer roles, counters) wait for the last piece.
struct PieceCtl { bool skip, finish; };
inline PieceCtl piece_ctl(pdlp_handle h, const Schedule& s, bool product_is_launched = true)
{
    const bool piece_mode = h->range_sel >= 0;
    const bool capable = product_is_launched && s.tiled && s.pending && s.nrange > 1;
    return PieceCtl{piece_mode && !capable && h->range_sel > 0, !piece_mode || h->range_sel >= h->range_cnt - 1};
}

// direct exchange: where the other ranks keep vector `v` (0 xbar, 1 / 2 / 3 the y buffers, 4 gdx, 5 gdy), at this rank's block
// (the half-steps pick the epilogue instantiation WITH the table only while h->peer.active: iterate_peer)
template <typename T> void peer_targets(pdlp_handle h, PeerOut<T, true>& po, int v)
{
    for (int i = 0; i < h->peer.n; ++i) po.p[i] = (T*)h->peer.out[v][i];
    po.n = h->peer.n;
}
template <typename T> void peer_targets(pdlp_handle, PeerOut<T, false>&, int) {}

template <typename T> T* xloc(pdlp_handle h, int ix) { return (T*)h->xb[ix] + h->p.col0; }
template <typename T> T* yloc(pdlp_handle h, int ix) { return (T*)h->yb[ix] + h->p.row0; }

// ---- launches shared by the half-steps, the KKT pass, the report and delta mode -----------------------------------------------
// which buffer triple holds iterate `which` (PDLP_CUR / PDLP_AVG / PDLP_PREV), -1: no such iterate
inline int iterate_index(pdlp_handle h, int which)
{
    return which == PDLP_CUR ? h->ix_cur : (which == PDLP_AVG ? h->ix_avg : (which == PDLP_PREV ? h->ix_prev : -1));
}

// A fused epilogue over `rows` rows without a matrix pass: over a vector of finished products (KKT sums from running products, a K'y
// kept by a check, the anchors of delta mode) or, with products == nullptr, over what the functor itself reads (report, delta mode's
// primal update).  Partial sums of rows_grid(rows) workgroups.
template <typename T, class Epi> int epilogue_pass(pdlp_handle h, int64_t rows, const void* products, Epi e, double* partials)
{
    if (rows == 0) return PDLP_OK;
    hipLaunchKernelGGL((k_rowsum_epilogue<T, Epi>), dim3(grid_for(rows)), dim3(BLOCK), 0, h->stream, (const T*)products, products ? 1 : 0,
                       (int64_t)0, (int)rows, (const T*)nullptr, e, partials);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// the end of a KKT pass: four sums of the gridA workgroups' partials (dual side) into red[0..3], two of gridB's (primal side) into red[4..5]
inline int finalize_kkt(pdlp_handle h, int gridA, int gridB)
{
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, h->stream, h->partA, gridA, 4, h->red, 0);
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, h->stream, h->partB, gridB, 2, h->red, 4);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// the step-size rule from the partial sums of the last primal and dual launch (advance: also count the iteration -- the library's
// own loop; 0: pdlp_adaptive_reduce, the caller's all-reduce and pdlp_adaptive_update follow)
inline void launch_adaptive_rule(pdlp_handle h, int advance)
{
    WITH_T(h->p.dtype, hipLaunchKernelGGL(k_adaptive_reduce_update<T>, dim3(1), dim3(BLOCK), 0, h->stream, h->partA, h->last_gridA, h->partB,
                                          h->last_gridB, h->red, h->sc, advance, (const double*)nullptr, 0));
}

// ... with the curvature of the step product among the sums (pdlp_objective_iterate: always the library's own loop)
inline void launch_objective_rule(pdlp_handle h)
{
    WITH_T(h->p.dtype, hipLaunchKernelGGL((k_adaptive_reduce_update<T, true>), dim3(1), dim3(BLOCK), 0, h->stream, h->partA, h->last_gridA,
                                          h->partB, h->last_gridB, h->red, h->sc, 1, (const double*)h->obj_mat.part, grid_of(h->sQ, h->nl)));
}

// f(flags...) with run-time switches as types (std::true_type / std::false_type), in the order given: with_flags(f, a, b) calls
// f(A, B).  A call site passes exactly the switches that vary there, so it instantiates f for their combinations and no others.
template <class F> int with_flags(F f) { return f(); }
template <class F, class... Rest> int with_flags(F f, bool flag, Rest... rest)
{
    return with_flags([&](auto... t) { return flag ? f(std::true_type{}, t...) : f(std::false_type{}, t...); }, rest...);
}

// the optional operand of a RANGED / QUAD functor (an empty member otherwise)
template <typename T> void set_optional(RowUpper<T, true>& o, pdlp_handle h) { o.p = (const T*)h->q_upper; }
template <typename T> void set_optional(ObjDiag<T, true>& o, pdlp_handle h) { o.p = (const T*)h->obj_diag; }
template <typename T> void set_optional(RowUpper<T, false>&, pdlp_handle) {}
template <typename T> void set_optional(ObjDiag<T, false>&, pdlp_handle) {}

// ---- the objective's matrix Q (pdlp_set_objective_matrix) -----------------------------------------------------------------------
// A product with Q over its own schedule and the caller's arrays, in the working type; the CSR form only (Q has neither tiles nor a
// sorted copy, and no epilogue of its own is built for the tiled kernels).  Q is a matrix of a whole problem on one GPU: no split
// product is ever pending on such a handle.
template <typename T, class Epi> int launch_obj_matrix(pdlp_handle h, const void* vin, Epi epi, double* partials)
{
    if (h->sQ.nblk == 0) return PDLP_OK;
    launch_csr_rows<T, T, Epi, false>(h, h->sQ, h->obj_mat.colidx, (const T*)h->obj_mat.val, vin, epi, partials);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// what the variable-side functors read as the objective's linear term: c, or the gradient g = c + Q x that obj_gradient has just formed
template <typename T> const T* obj_linear(pdlp_handle h) { return h->obj_mat.on ? (const T*)h->lam_prev : (const T*)h->p.c; }

// g = c + Q x of iterate buffer `ix` into the gradient buffer; SUM: also x'Qx into red[OBJ_XQX], through partA (before the pass that
// follows reuses it: the stream orders the two)
template <typename T, bool SUM> int obj_gradient(pdlp_handle h, int ix)
{
    ObjGradEpi<T, SUM> e{(const T*)h->p.c, xloc<T>(h, ix), (T*)h->lam_prev};
    const int rc = launch_obj_matrix<T>(h, h->xb[ix], e, h->partA);
    if (rc != PDLP_OK || !SUM) return rc;
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, h->stream, h->partA, grid_of(h->sQ, h->nl), 1, h->red, (int)pdlp_solver::OBJ_XQX);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// The step product of the adaptive iteration (pdlp_objective_iterate), behind its primal half-step: g = c + Q x' of the NEW x (still
// in the "previous" buffers: the dual half-step swaps the roles) over the g of the old x, and the partial sums of the curvature
// dx'Q dx into the handle's own array -- partA holds ||dx||^2 and partB will hold the dual half's sums when the rule reads all three
template <typename T> int obj_gradient_step(pdlp_handle h)
{
    ObjGradStepEpi<T> e{(const T*)h->p.c, xloc<T>(h, h->ix_prev), xloc<T>(h, h->ix_cur), (T*)h->lam_prev};
    return launch_obj_matrix<T>(h, h->xb[h->ix_prev], e, h->obj_mat.part);
}

// the end of a KKT pass or report over g: the objective's slots from g'x to the contract's c'x + 1/2 x'Qx (k_obj_matrix_finish)
inline int obj_matrix_finish(pdlp_handle h)
{
    hipLaunchKernelGGL(k_obj_matrix_finish, dim3(1), dim3(1), 0, h->stream, h->red, (int)pdlp_solver::OBJ_XQX);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

template <typename T> int obj_product_t(pdlp_handle h, const void* x_full, void* out_local)
{
    StoreEpi<T> e{(T*)out_local};
    return launch_obj_matrix<T>(h, x_full, e, h->partA);
}

// QUAD: the handle has a diagonal quadratic objective (pdlp_set_objective_diag: float32 / float64, one GPU, no exchange -- so never
// PEER)
template <typename T, bool ADAPT, bool PEER, bool QUAD = false> int primal_half_e(pdlp_handle h, int src, T* ksum, const PieceCtl& pc)
{
    PrimalEpi<T, ADAPT, PEER, QUAD> e{xloc<T>(h, h->ix_cur), xloc<T>(h, h->ix_prev), (T*)h->xbar + h->p.col0, obj_linear<T>(h),
                                      (const T*)h->p.l, (const T*)h->p.u, (T*)h->x_sum, h->sc, ksum};
    peer_targets(h, e.peer, 0);
    set_optional(e.diag, h);
    if (src >= 0) {     // the primal update from a K'y that a KKT pass at this very iterate left behind: no product, one vector kernel
        if (ADAPT) h->last_gridA = rows_grid(h->nl);
        return epilogue_pass<T>(h, h->nl, h->ktyb[src], e, h->partA);
    }
    if (ADAPT) h->last_gridA = grid_of(h->sKT, h->nl);
    h->use_split = true;
    const int rc = launch_csr<T>(h, true, h->yb[h->ix_cur], e, h->partA);
    h->use_split = false;
    if (pc.finish) h->sKT.pending = false;
    return rc;
}

template <typename T> int primal_half_t(pdlp_handle h, int adaptive)
{
    // K'y of the current iterate may still be there from the restart check (of the current iterate if nothing moved
    // since, or of the candidate the restart adopted)
    const Carried& c = h->carry;
    const int src = (h->no_kty_reuse || h->graph_ok || h->sKT.pending) ? -1 : (c.kty_cur >= 0 ? c.kty_cur : (c.cand_cur != CAND_NONE ? 0 : -1));
    // K'y of the previous iterate's y joins the running sum unless this is the first half-step after a reset (that y is the
    // restart point) or the restart check's flush has already added it
    // (not under graph replay: a captured launch would freeze this decision)
    T* ksum = (c.since_reset > 0 && !c.kty_tail_done && !c.sums_broken && !h->no_running && !h->graph_ok) ? (T*)h->kty_sum : nullptr;
    const PieceCtl pc = piece_ctl(h, h->sKT, src < 0);
    if (pc.skip) return PDLP_OK;                             // (all of this half-step went out with piece 0)
    // sparse quadratic objective: the linearised step takes the gradient c + Q x of the current x where it takes c -- one more product
    // ahead of EVERY primal half-step, the vector-pass form over a kept K'y included.  (The adaptive half-step reaches this function
    // from pdlp_objective_iterate alone, which has seen to the gradient itself: carried from its last step product, or formed.)
    if (h->obj_mat.on && !adaptive) {
        const int rc = obj_gradient<T, false>(h, h->ix_cur);
        if (rc != PDLP_OK) return rc;
        h->carry.gradient_overwritten();       // (g of the x this half-step leaves)
    }
    if (h->obj_diag) return with_flags([&](auto A) { return primal_half_e<T, A.value, false, true>(h, src, ksum, pc); }, adaptive);
    // (inside the direct exchange the epilogue also stores xbar into the peers: its own instantiations)
    return with_flags([&](auto A, auto P) { return primal_half_e<T, A.value, P.value>(h, src, ksum, pc); }, adaptive, h->peer.active);
}

template <typename T> int refresh_kx_t(pdlp_handle h)
{
    StoreEpi<T> e{(T*)h->kxb[0]};
    int rc = launch_csr<T>(h, false, h->xb[h->ix_cur], e, h->partB);
    if (rc == PDLP_OK) h->carry.kx_refreshed();
    return rc;
}

// RANGED: the handle has two-sided rows (pdlp_set_row_upper: float32 / float64, one GPU, no exchange -- so never PEER)
template <typename T, bool ADAPT, bool PEER, bool RANGED = false> int dual_half_e(pdlp_handle h, T* ksum)
{
    DualEpi<T, ADAPT, PEER, RANGED> e{yloc<T>(h, h->ix_cur), yloc<T>(h, h->ix_prev), (const T*)h->p.q, (T*)h->y_sum, (T*)h->kxb[0],
                                      h->sc, h->ineq_end, ksum};
    peer_targets(h, e.peer, 1 + h->ix_prev);
    set_optional(e.upper, h);
    if (ADAPT) h->last_gridB = grid_of(h->sK, h->ml);
    h->use_split = true;
    const int rc = launch_csr<T>(h, false, h->xbar, e, h->partB);
    h->use_split = false;
    return rc;
}

template <typename T> int dual_half_t(pdlp_handle h, int adaptive)
{
    int rc;
    if (!h->carry.kx_valid && (rc = refresh_kx_t<T>(h)) != PDLP_OK) return rc;      // K x of the current x: carried along from here on
    T* ksum = (h->carry.sums_broken || h->no_running || h->graph_ok) ? nullptr : (T*)h->kx_sum;
    const PieceCtl pc = piece_ctl(h, h->sK);
    rc = PDLP_OK;
    if (!pc.skip && h->q_upper)
        rc = with_flags([&](auto A) { return dual_half_e<T, A.value, false, true>(h, ksum); }, adaptive);
    else if (!pc.skip)       // (else: all of this half-step went out with piece 0)
        rc = with_flags([&](auto A, auto P) { return dual_half_e<T, A.value, P.value>(h, ksum); }, adaptive, h->peer.active);
    if (rc != PDLP_OK) { h->sK.pending = false; return rc; }
    if (!pc.finish) return PDLP_OK;                          // (more pieces of this half-step to come)
    h->sK.pending = false;
    const int t = h->ix_cur;   // the freshly written buffers become current, the old ones previous
    h->ix_cur = h->ix_prev;
    h->ix_prev = t;
    h->carry.iterated(1, false);
    return PDLP_OK;
}

template <typename T> int half_begin_t(pdlp_handle h, bool transpose, const void* vin)
{
    Schedule& s = transpose ? h->sKT : h->sK;
    if (!s.tiled || s.slotsA == 0 || (!h->gstream && !h->begin_inline) || s.pending) return PDLP_OK;
    const int rows = (int)(transpose ? h->nl : h->ml);
    // begin_inline (PDLP_OPT_BEGIN_INLINE): the caller has ALREADY issued the exchange asynchronously on a stream of its own, so the
    // local panels simply go onto the handle's stream and run beside it -- no side stream, no fork / join events (each cross-stream
    // dependency costs about a kernel launch on this stack); the half-step that follows then has nothing to wait for
    hipStream_t st = h->begin_inline ? h->stream : h->gstream;
    if (!h->begin_inline) {
        HIP_TRY(hipEventRecord(h->ev_in, h->stream));
        HIP_TRY(hipStreamWaitEvent(h->gstream, h->ev_in, 0));
    }
    if (h->delta) launch_phase<float, float>(h, s, rows, transpose ? (const void*)h->gdy : (const void*)h->gdx, st, 0);
    else if (std::is_same<T, double>::value && h->mixed) launch_phase<double, float>(h, s, rows, vin, st, 0);
    else launch_phase<T, T>(h, s, rows, vin, st, 0);
    if (!h->begin_inline) HIP_TRY(hipEventRecord(h->ev_out, h->gstream));
    HIP_TRY(hipGetLastError());
    s.pending = true;
    s.pending_inline = h->begin_inline;
    s.chunks_done = 0;
    return PDLP_OK;
}

// the panels that chunk `chunk` of the exchange completes, on the handle's stream (the caller has made that stream wait for the
// chunk); the last chunk's panels are launched by the half-step itself, together with the sum and the epilogue
template <typename T> int half_chunk_t(pdlp_handle h, bool transpose, const void* vin, int chunk)
{
    Schedule& s = transpose ? h->sKT : h->sK;
    if (!s.pending || s.nphase == 0) return PDLP_OK;           // the product is not split this time: the half-step does it all
    if (chunk != s.chunks_done || chunk + 2 >= s.nphase + 0) return chunk + 2 == s.nphase ? PDLP_OK : PDLP_ERR_STATE;
    const int rows = (int)(transpose ? h->nl : h->ml);
    if (h->delta) launch_phase<float, float>(h, s, rows, transpose ? (const void*)h->gdy : (const void*)h->gdx, h->stream, 1 + chunk);
    else if (std::is_same<T, double>::value && h->mixed) launch_phase<double, float>(h, s, rows, vin, h->stream, 1 + chunk);
    else launch_phase<T, T>(h, s, rows, vin, h->stream, 1 + chunk);
    HIP_TRY(hipGetLastError());
    ++s.chunks_done;
    return PDLP_OK;
}

template <typename T> int spmv_t(pdlp_handle h, int transpose, const void* in_full, void* out_local)
{
    StoreEpi<T> e{(T*)out_local};
    return launch_csr<T>(h, transpose != 0, in_full, e, h->partA);
}

// One output piece of a half-step (see pdlp_hip.h).  Pieces in order, 0 .. pieces-1; the half-step is complete after the last.
int half_piece(pdlp_handle h, bool dual, int adaptive, int piece, int pieces)
{
    if (!h || pieces < 1 || pieces > MAX_CHUNKS || piece < 0 || piece >= pieces) return PDLP_ERR_INVALID;
    h->range_sel = piece;
    h->range_cnt = pieces;
    const int rc = dual ? pdlp_dual_half(h, adaptive) : pdlp_primal_half(h, adaptive);
    h->range_sel = -1;
    h->range_cnt = 1;
    return rc;
}

}  // namespace
