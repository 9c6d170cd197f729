// pdlp_driver.inc -- the library's own iteration driver, the three forms pdlp_iterate chooses from besides the direct exchange:
// iterate_direct (plain launches), iterate_single (one GPU: optionally two captured iterations replayed as a hipGraph) and
// iterate_sharded (the exchange inside the library over RCCL: all-gathers, or grouped broadcasts chunk by chunk on a communication
// stream while the handle's stream multiplies what has arrived); and the pdlp_comm_* entry points that own the communicator.
// Part of pdlp_hip.hip (included at file scope; not a translation unit of its own).  Needs: pdlp_products.inc (half_piece),
// pdlp_delta.inc (delta_refresh), pdlp_schedule.inc (plan_bounds), pdlp_loaders.inc; calls the half-steps through the ABI.
// ------------------------------------------------------------------------------------------------
namespace {

int iterate_direct(pdlp_handle h, int iters, int adaptive)
{
    int rc;
    for (int it = 0; it < iters; ++it) {
        if ((rc = pdlp_primal_half(h, adaptive)) != PDLP_OK) return rc;
        if ((rc = pdlp_dual_half(h, adaptive)) != PDLP_OK) return rc;
        if (adaptive) launch_adaptive_rule(h, 1);
    }
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// Graph replay was asked for (PDLP_GRAPH) and cannot be had: say so once per process -- the iteration falls back to plain launches,
// which is correct but slower on small LPs, and would otherwise show up only as a slower benchmark.
// The running sums were not kept while replay was on: no running average before the next restart.
pdlp_solver::IterGraph* graph_abandoned(pdlp_handle h, const char* why)
{
    static bool said = false;
    if (!said) std::fprintf(stderr, "libpdlp_hip: PDLP_GRAPH: graph capture abandoned (%s); iterating with direct launches\n", why);
    said = true;
    h->graph_ok = false;
    h->carry.sums_end();
    return nullptr;
}

// the executable graph of two iterations from the current buffer roles (captured on first use), or nullptr
pdlp_solver::IterGraph* pair_graph(pdlp_handle h, int adaptive)
{
    pdlp_solver::IterGraph* slot = nullptr;
    for (auto& g : h->graphs) {
        if (g.valid && g.ix_cur == h->ix_cur && g.ix_prev == h->ix_prev && g.adaptive == adaptive) return &g;
        if (!g.valid && !slot) slot = &g;
    }
    if (!slot) return nullptr;
    // capture: the launch code runs unchanged against the library's stream; the host-side roles and the whole carried state are
    // put back afterwards -- a capture issues launches and leaves no trace (replayed() accounts for the replays)
    const int ix_cur = h->ix_cur, ix_prev = h->ix_prev, gA = h->last_gridA, gB = h->last_gridB;
    const Carried carry = h->carry;
    hipStream_t user = h->stream;
    if (hipStreamBeginCapture(h->gstream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        return graph_abandoned(h, "hipStreamBeginCapture failed");
    }
    h->stream = h->gstream;
    const int rc = iterate_direct(h, 2, adaptive);
    h->stream = user;
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(h->gstream, &graph);
    h->ix_cur = ix_cur; h->ix_prev = ix_prev; h->last_gridA = gA; h->last_gridB = gB;
    h->carry = carry;
    if (rc != PDLP_OK || e != hipSuccess || !graph ||
        hipGraphInstantiate(&slot->exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        return graph_abandoned(h, rc != PDLP_OK ? "a launch failed during capture" : "hipStreamEndCapture / hipGraphInstantiate failed");
    }
    (void)hipGraphDestroy(graph);
    slot->valid = true; slot->ix_cur = ix_cur; slot->ix_prev = ix_prev; slot->adaptive = adaptive;
    return slot;
}

// all-gather of a full-length vector whose block of this rank is in place (equal blocks: rank r's block starts at r * count)
int comm_all_gather(pdlp_handle h, void* full, int64_t count, bool f32)
{
    char* base = (char*)full;
    const size_t esz = f32 ? 4 : 8;
    RCCL_TRY(g_rccl.AllGather(base + (size_t)h->comm_rank * count * esz, base, (size_t)count, f32 ? ncclFloat32 : ncclFloat64, h->comm,
                              h->stream));
    return PDLP_OK;
}

// the exchange of one gathered vector in the chunks of its product's plan: chunk c = elements [sb[c], sb[c+1]) of every rank's
// block, as one group of in-place broadcasts (one root per rank) on the communication stream; ev_chunk[c] marks its arrival
int comm_exchange_piece(pdlp_handle h, int c, const int64_t* sb, void* full, int64_t block, bool f32, hipEvent_t ready)
{
    const size_t esz = f32 ? 4 : 8;
    if (g_roctx.level > 0 && g_roctx.push) (void)g_roctx.push("pdlp: exchange piece (grouped broadcasts issued)");
    struct Pop { ~Pop() { if (g_roctx.level > 0 && g_roctx.pop) (void)g_roctx.pop(); } } pop_;
    HIP_TRY(hipStreamWaitEvent(h->cstream, ready, 0));          // this rank's part of the piece is final
    const int64_t lo = sb[c], cnt = sb[c + 1] - sb[c];
    if (cnt > 0) {
        RCCL_TRY(g_rccl.GroupStart());
        for (int q = 0; q < h->comm_size; ++q) {
            char* ptr = (char*)full + ((size_t)q * block + lo) * esz;
            const ncclResult_t r = g_rccl.Broadcast(ptr, ptr, (size_t)cnt, f32 ? ncclFloat32 : ncclFloat64, q, h->comm, h->cstream);
            if (r != ncclSuccess) { (void)g_rccl.GroupEnd(); g_rccl.last_error = (int)r; return PDLP_ERR_COMM; }
        }
        RCCL_TRY(g_rccl.GroupEnd());
    }
    HIP_TRY(hipEventRecord(h->ev_chunk[c], h->cstream));
    return PDLP_OK;
}

int comm_exchange_chunked(pdlp_handle h, int C, const int64_t* sb, void* full, int64_t block, bool f32)
{
    const size_t esz = f32 ? 4 : 8;
    HIP_TRY(hipEventRecord(h->ev_vec, h->stream));               // this rank's block is final
    HIP_TRY(hipStreamWaitEvent(h->cstream, h->ev_vec, 0));
    for (int c = 0; c < C; ++c) {
        const int64_t lo = sb[c], cnt = sb[c + 1] - sb[c];
        if (cnt > 0) {
            RCCL_TRY(g_rccl.GroupStart());
            for (int q = 0; q < h->comm_size; ++q) {
                char* ptr = (char*)full + ((size_t)q * block + lo) * esz;
                const ncclResult_t r = g_rccl.Broadcast(ptr, ptr, (size_t)cnt, f32 ? ncclFloat32 : ncclFloat64, q, h->comm, h->cstream);
                if (r != ncclSuccess) { (void)g_rccl.GroupEnd(); g_rccl.last_error = (int)r; return PDLP_ERR_COMM; }
            }
            RCCL_TRY(g_rccl.GroupEnd());
        }
        HIP_TRY(hipEventRecord(h->ev_chunk[c], h->cstream));
    }
    return PDLP_OK;
}

// one half-step of a sharded iteration with the exchange of its input in front: K xbar (transpose 0) or K'y (1, not after the
// last iteration of the call).  Chunked plans: the chunks travel on the communication stream, and the handle's stream multiplies
// the panels a chunk completes as soon as it has arrived; the last chunk's panels, the sum and the epilogue are the half-step.
int sharded_exchange_and_begin(pdlp_handle h, bool transpose, int adaptive, bool begin, bool pieces_sent = false)
{
    int rc;
    const bool vec32 = h->p.dtype == PDLP_F32;
    void* full = transpose ? (h->delta ? (void*)h->gdy : (void*)h->yb[h->ix_cur]) : (h->delta ? (void*)h->gdx : (void*)h->xbar);
    const int64_t block = transpose ? h->ml : h->nl;
    const bool f32 = h->delta || vec32;
    // the panels that meet this rank's own block are multiplied while the other blocks are on the wire: on the handle's own stream when
    // the pieces are under way on the communication stream already, else on the side stream (the all-gather below is in stream order)
    const bool saved_inline = h->begin_inline;
    h->begin_inline = pieces_sent;
    rc = begin ? (transpose ? pdlp_primal_half_begin(h) : pdlp_dual_half_begin(h, adaptive)) : PDLP_OK;
    h->begin_inline = saved_inline;
    if (rc != PDLP_OK) return rc;
    // (the shape of the exchange must not depend on anything rank local -- every rank issues the same collectives)
    int64_t sb[MAX_PHASE];
    const int C = plan_bounds(block, h->xchunks, sb);
    const bool chunked = C > 1 && h->cstream && g_rccl.Broadcast && g_rccl.GroupStart && g_rccl.GroupEnd;
    if (!chunked) return comm_all_gather(h, full, block, f32);
    // (pieces_sent: the half-step that produced the vector was issued piece by piece and every piece's broadcasts went out behind
    //  its rows -- sharded_half_in_pieces; only the consumer's side is left to do)
    if (!pieces_sent && (rc = comm_exchange_chunked(h, C, sb, full, block, f32)) != PDLP_OK) return rc;
    for (int c = 0; c + 1 < C; ++c) {
        HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_chunk[c], 0));
        if ((rc = pdlp_half_chunk(h, transpose ? 1 : 0, c)) != PDLP_OK) return rc;
    }
    HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_chunk[C - 1], 0));
    return PDLP_OK;
}

// A half-step whose result travels in pieces: piece r's rows (last phase of the product + epilogue), an event, and piece r's
// broadcasts on the communication stream behind that event -- they run while piece r + 1's rows are still being multiplied.
// Returns (through *sent) whether the pieces went out this way; if not, the caller exchanges the vector after the half-step.
// The shape of the collectives is the plan's alone: every rank issues the same groups whether or not its own product is split.
int sharded_half_in_pieces(pdlp_handle h, bool dual, int adaptive, bool* sent)
{
    int rc;
    *sent = false;
    const bool vec32 = h->p.dtype == PDLP_F32;
    // the vector this half-step writes and the exchange it feeds: primal -> xbar (input of K xbar), dual -> y (input of K'y)
    void* full = dual ? (h->delta ? (void*)h->gdy : (void*)h->yb[h->ix_prev]) : (h->delta ? (void*)h->gdx : (void*)h->xbar);
    const int64_t block = dual ? h->ml : h->nl;
    const bool f32 = h->delta || vec32;
    int64_t sb[MAX_PHASE];
    const int C = plan_bounds(block, h->xchunks, sb);
    const bool chunked = C > 1 && h->cstream && h->producer_pieces && g_rccl.Broadcast && g_rccl.GroupStart && g_rccl.GroupEnd;
    if (!chunked) return dual ? pdlp_dual_half(h, adaptive) : pdlp_primal_half(h, adaptive);
    for (int c = 0; c < C; ++c) {
        if ((rc = half_piece(h, dual, adaptive, c, C)) != PDLP_OK) return rc;
        HIP_TRY(hipEventRecord(h->ev_row[c], h->stream));
        if ((rc = comm_exchange_piece(h, c, sb, full, block, f32, h->ev_row[c])) != PDLP_OK) return rc;
    }
    *sent = true;
    return PDLP_OK;
}

// the iterations of a sharded problem with the exchange inside the library: the same sequence as PdlpEngine.iterate drives
// through torch.distributed (engine.py), all of it enqueued on the handle's streams -- one call per restart period, no host
// work between the kernels and the collectives
int iterate_sharded(pdlp_handle h, int iters, int adaptive)
{
    int rc;
    const bool vec32 = h->p.dtype == PDLP_F32;
    if (h->delta && iters > 0 && !h->carry.anchors_valid) {
        if ((rc = comm_all_gather(h, h->xb[h->ix_cur], h->nl, vec32)) != PDLP_OK) return rc;
        if ((rc = comm_all_gather(h, h->yb[h->ix_cur], h->ml, vec32)) != PDLP_OK) return rc;
        if ((rc = delta_refresh(h)) != PDLP_OK) return rc;
    }
    for (int it = 0; it < iters; ++it) {
        bool sent = false;
        if ((rc = sharded_half_in_pieces(h, false, adaptive, &sent)) != PDLP_OK) return rc;
        if ((rc = sharded_exchange_and_begin(h, false, adaptive, true, sent)) != PDLP_OK) return rc;      // xbar (delta mode: x+ - x)
        if ((rc = sharded_half_in_pieces(h, true, adaptive, &sent)) != PDLP_OK) return rc;
        // the step-size rule's three sums: with the pieces on the communication stream the all-reduce queues up behind them there
        // and runs while the handle's stream multiplies the panels the pieces complete (same sums, same values: only the order in
        // which independent work is enqueued changes)
        const bool ar_early = adaptive && sent && h->ev_ar;
        // (the kernel that adds up this rank's three sums needs only the half-steps' partial sums: it runs while y is on the wire)
        if (adaptive && (rc = pdlp_adaptive_reduce(h)) != PDLP_OK) return rc;
        if (ar_early) {
            HIP_TRY(hipEventRecord(h->ev_vec, h->stream));
            HIP_TRY(hipStreamWaitEvent(h->cstream, h->ev_vec, 0));
            RCCL_TRY(g_rccl.AllReduce(h->red, h->red, 3, ncclFloat64, ncclSum, h->comm, h->cstream));
            HIP_TRY(hipEventRecord(h->ev_ar, h->cstream));
        }
        // the new y (delta mode: y+ - y) -- final: a rejected adaptive step is kept, quirk Q1; its product starts only if
        // another iteration follows in this call
        if ((rc = sharded_exchange_and_begin(h, true, adaptive, it + 1 < iters, sent)) != PDLP_OK) return rc;
        if (ar_early) {
            HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_ar, 0));
            if ((rc = pdlp_adaptive_update(h)) != PDLP_OK) return rc;
        } else if (adaptive) {
            RCCL_TRY(g_rccl.AllReduce(h->red, h->red, 3, ncclFloat64, ncclSum, h->comm, h->stream));
            if ((rc = pdlp_adaptive_update(h)) != PDLP_OK) return rc;
        }
    }
    if (!adaptive && iters > 0) return pdlp_fixed_advance(h, iters);
    return PDLP_OK;
}

// pdlp_objective_iterate: the adaptive iteration of the linearised step (sparse quadratic objective; one GPU, plain launches).  The
// product with Q sits BEHIND the primal half-step, at x': its epilogue has g(x) and g(x') of a row side by side and sums the
// curvature dx'Q dx for the rule, and -- a rejected trial is kept -- g(x') is the gradient the next iteration's half-step reads.
// Three products per iteration, as the fixed step has; the gradient is formed ahead of the half-step only where nothing carried it
// (Carried::g_cur: the first iteration, after a KKT pass, a restart, fixed iterations).
template <typename T> int objective_iterate_t(pdlp_handle h, int iters)
{
    int rc;
    for (int it = 0; it < iters; ++it) {
        if (!h->carry.g_cur && (rc = obj_gradient<T, false>(h, h->ix_cur)) != PDLP_OK) return rc;
        if ((rc = primal_half_t<T>(h, 1)) != PDLP_OK) return rc;
        h->carry.gradient_overwritten();       // (from here the buffer holds g(x') while x is still current: down until the swap succeeds)
        if ((rc = obj_gradient_step<T>(h)) != PDLP_OK) return rc;
        if ((rc = dual_half_t<T>(h, 1)) != PDLP_OK) return rc;
        h->carry.gradient_stepped();
        launch_objective_rule(h);
    }
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// the iterations of a problem on one GPU: direct launches, or (PDLP_OPT_GRAPH) pairs of iterations replayed from a captured graph
int iterate_single(pdlp_handle h, int iters, int adaptive)
{
    int rc, left = iters;
    if (h->graph_ok && left >= 5) {
        if (!h->carry.kx_valid) {    // the first iteration after a reset also refreshes the K x cache: never inside a captured pair
            if ((rc = iterate_direct(h, 1, adaptive)) != PDLP_OK) return rc;
            --left;
        }
        pdlp_solver::IterGraph* g = pair_graph(h, adaptive);
        if (g) {
            const int pairs = left / 2;
            HIP_TRY(hipEventRecord(h->ev_in, h->stream));
            HIP_TRY(hipStreamWaitEvent(h->gstream, h->ev_in, 0));
            for (; left >= 2; left -= 2) HIP_TRY(hipGraphLaunch(g->exec, h->gstream));
            HIP_TRY(hipEventRecord(h->ev_out, h->gstream));
            HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_out, 0));
            h->carry.replayed(pairs, h->delta);              // (what that many direct iterations leave behind)
            if (adaptive) { h->last_gridA = grid_of(h->sKT, h->nl); h->last_gridB = grid_of(h->sK, h->ml); }
        }
    }
    if ((rc = iterate_direct(h, left, adaptive)) != PDLP_OK) return rc;
    if (!adaptive && iters > 0) return pdlp_fixed_advance(h, iters);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

}  // namespace

extern "C" {

int pdlp_comm_load(const char* rccl_path) { return rccl_load(rccl_path); }

int pdlp_comm_unique_id(const char* rccl_path, void* id128)
{
    if (!id128) return PDLP_ERR_INVALID;
    const int rc = rccl_load(rccl_path);
    if (rc != PDLP_OK) return rc;
    ncclUniqueId id;
    RCCL_TRY(g_rccl.GetUniqueId(&id));
    std::memcpy(id128, &id, sizeof(id));
    return PDLP_OK;
}

int pdlp_comm_init(pdlp_handle h, const char* rccl_path, const void* id128, int rank, int nranks)
{
    if (!h || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return PDLP_ERR_INVALID;
    // equal blocks, this rank's at rank * block (the padded layout of torchpdlp_amd/distributed.py)
    if (h->nl * nranks != h->p.n || h->ml * nranks != h->p.m || h->p.col0 != (int64_t)rank * h->nl || h->p.row0 != (int64_t)rank * h->ml)
        return PDLP_ERR_INVALID;
    if (has_extension(h)) return PDLP_ERR_STATE;      // (two-sided rows and the quadratic term have no sharded form)
    const int rc = rccl_load(rccl_path);
    if (rc != PDLP_OK) return rc;
    if (h->comm) { (void)g_rccl.CommDestroy(h->comm); h->comm = nullptr; }
    HIP_TRY(hipSetDevice(h->p.device));
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    RCCL_TRY(g_rccl.CommInitRank(&h->comm, nranks, id, rank));
    h->comm_rank = rank; h->comm_size = nranks;
    if (!h->cstream) {           // (chunked exchange: without these it stays one all-gather on the handle's stream)
        bool ok = hipStreamCreateWithFlags(&h->cstream, hipStreamNonBlocking) == hipSuccess &&
                  hipEventCreateWithFlags(&h->ev_vec, hipEventDisableTiming) == hipSuccess;
        for (auto& e : h->ev_chunk) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        for (auto& e : h->ev_row) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&h->ev_ar, hipEventDisableTiming) == hipSuccess;
        if (!ok) { if (h->cstream) (void)hipStreamDestroy(h->cstream); h->cstream = nullptr; (void)hipGetLastError(); }
    }
    return PDLP_OK;
}

int pdlp_comm_all_gather(pdlp_handle h, int which)
{
    if (!h || !h->comm) return PDLP_ERR_STATE;
    void* p = nullptr;
    const int rc = pdlp_buffer_ptr(h, which, &p);
    if (rc != PDLP_OK) return rc;
    const bool is_x = which <= PDLP_BUF_X_AVG || which == PDLP_BUF_DX || which == PDLP_BUF_GDX;
    if (which == PDLP_BUF_RED || which == PDLP_BUF_SCALARS || which == PDLP_BUF_X_SUM || which == PDLP_BUF_Y_SUM || which == PDLP_BUF_LAM_PREV)
        return PDLP_ERR_INVALID;
    const bool f32 = h->p.dtype == PDLP_F32 || which == PDLP_BUF_GDX || which == PDLP_BUF_GDY;
    return comm_all_gather(h, p, is_x ? h->nl : h->ml, f32);
}

int pdlp_comm_all_reduce_red(pdlp_handle h)
{
    if (!h || !h->comm) return PDLP_ERR_STATE;
    RCCL_TRY(g_rccl.AllReduce(h->red, h->red, PDLP_NRED, ncclFloat64, ncclSum, h->comm, h->stream));
    return PDLP_OK;
}

}  // extern "C"
