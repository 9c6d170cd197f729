// pdlp_peer.inc -- the direct exchange of a sharded problem on one node: no collective in the iteration.  A half-step's epilogue
// stores its block into every peer's copy of the vector (the peers' workspaces are opened over HIP IPC), tiny kernels raise and
// await flags in fine-grained mailboxes (peer_signal, peer_wait, the push form's copy kernel), iterate_peer is the loop; and the
// pdlp_peer_* entry points that export, connect, report and close.
// Part of pdlp_hip.hip (included at file scope; not a translation unit of its own).  Needs: pdlp_handle.inc (pdlp_solver::Peer,
// peer_release); calls the half-steps through the ABI.
// (ADVICE.md, open and left as it is: iterate_peer leaves its loop on an error after P.seq has advanced, without resynchronising
// with the peers.)
// ------------------------------------------------------------------------------------------------
namespace {

// "everything this rank has stored into your vectors up to now is complete" to every peer (and, with_sums, this rank's three sums of
// the step-size rule): one tiny kernel behind the half-step that did the storing
int peer_signal(pdlp_handle h, bool with_sums, hipStream_t stream = nullptr)
{
    pdlp_solver::Peer& P = h->peer;
    if (!stream) stream = h->stream;
    PeerSignal sg{};
    for (int i = 0; i < P.n; ++i) { sg.flag[i] = P.flag[i]; sg.sums[i] = P.sums[i]; }
    sg.own_sums = (double*)(P.box + BOX_SUMS_AT) + (size_t)P.rank * BOX_SUMS_STRIDE;
    sg.own_flag = (uint32_t*)P.box + (size_t)P.rank * BOX_FLAG_STRIDE;
    sg.n = P.n;
    sg.seq = ++P.seq;
    if (!with_sums)
        hipLaunchKernelGGL(k_peer_signal, dim3(1), dim3(64), 0, stream, sg);
    else                                  // (pdlp_adaptive_reduce and the signal in one launch)
        WITH_T(h->p.dtype, hipLaunchKernelGGL(k_adaptive_reduce_signal<T>, dim3(1), dim3(BLOCK), 0, stream, h->partA, h->last_gridA, h->partB,
                                              h->last_gridB, h->red, h->sc, sg));
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// bytes per element of target vector v and the start of this rank's block in it
size_t peer_block_start(pdlp_handle h, int v)
{
    const size_t esz = v >= 4 ? 4 : h->es;
    return (size_t)(v == 0 || v == 4 ? h->p.col0 : h->p.row0) * esz;
}

// push form: behind everything the handle's stream has enqueued so far, on the side stream: this rank's block of vector v (0 xbar,
// 1..3 the y buffers, 4 gdx, 5 gdy) into every peer's copy, then the signal (with the step-size rule's sums for the y exchange)
int peer_push_and_signal(pdlp_handle h, int v, bool with_sums)
{
    pdlp_solver::Peer& P = h->peer;
    if (!P.pstream) {
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(&P.pstream, hipStreamNonBlocking, greatest));
        HIP_TRY(hipEventCreateWithFlags(&P.ev_push, hipEventDisableTiming));
    }
    HIP_TRY(hipEventRecord(P.ev_push, h->stream));
    HIP_TRY(hipStreamWaitEvent(P.pstream, P.ev_push, 0));
    const bool x_side = v == 0 || v == 4;
    const int64_t len = x_side ? h->nl : h->ml;
    const char* base = v == 0 ? h->xbar : (v == 4 ? (const char*)h->gdx : (v == 5 ? (const char*)h->gdy : h->yb[v - 1]));
    const char* src = base + peer_block_start(h, v);
    // (a modest grid: the copy is link-bound.  Where the own-block launch fills the chip -- 2 ranks: 502 workgroups holding every
    //  register of every CU -- the copy only gets going when those workgroups retire, and a grid small enough for the slots they
    //  leave is too slow to feed a link: measured, profiles/r05_multi_gpu/README.md.  The form pays at 4 ranks.)
    const int grid = (int)((len + BLOCK - 1) / BLOCK < 128 ? (len + BLOCK - 1) / BLOCK : 128);
    if (len > 0) {
        if (v >= 4 || h->es == 4) {
            PeerPush<float> d{};
            for (int i = 0; i < P.n; ++i) d.dst[i] = (float*)P.out[v][i];
            d.n = P.n;
            hipLaunchKernelGGL(k_peer_push<float>, dim3(grid), dim3(BLOCK), 0, P.pstream, (const float*)src, d, len);
        } else {
            PeerPush<double> d{};
            for (int i = 0; i < P.n; ++i) d.dst[i] = (double*)P.out[v][i];
            d.n = P.n;
            hipLaunchKernelGGL(k_peer_push<double>, dim3(grid), dim3(BLOCK), 0, P.pstream, (const double*)src, d, len);
        }
    }
    return peer_signal(h, with_sums, P.pstream);
}

// the handle's stream waits until every peer has signalled the exchange just signalled by this rank (bounded: k_peer_wait);
// then_update: the step-size rule from all ranks' sums in the same launch
int peer_wait(pdlp_handle h, bool then_update = false)
{
    pdlp_solver::Peer& P = h->peer;
    if (!then_update)
        hipLaunchKernelGGL(k_peer_wait, dim3(PEER_WAIT_BLOCKS), dim3(64), 0, h->stream, (const uint32_t*)P.box, P.world, P.rank, P.seq, P.limit_ticks, P.err_dev);
    else
        WITH_T(h->p.dtype, hipLaunchKernelGGL(k_peer_wait_adaptive_update<T>, dim3(PEER_WAIT_BLOCKS), dim3(64), 0, h->stream, (const uint32_t*)P.box,
                                              P.world, P.rank, P.seq, P.limit_ticks, P.err_dev, h->sc, h->red));
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

// The iterations of a sharded problem WITHOUT collectives: a half-step's epilogue stores its block of xbar / y (delta mode: of the
// float32 differences) into every peer's copy as it computes it (PeerOut), a one-wave kernel raises this rank's flag in the peers'
// mailboxes, a one-wave kernel waits for the peers' flags, and the next product follows (PDLP_OPT_PEER_LOCAL_FIRST: split, the panels
// that meet the own block between signal and wait -- cover for ranks that finish at different times, at the price of a launch that
// cannot fill the chip: the own block is 1/world of the panels).  The step-size rule's three sums travel with the flag of the y exchange and are added in rank
// order by every rank.  One stream, no events (the push form: a side stream for the copy kernel); per half-step the exchange adds two launches of a few microseconds to the critical
// path (tools/src/ipc_probe.hip: 5.8 us for the pair between two processes) where an all-gather adds its whole duration.
// Same arithmetic as iterate_sharded / PdlpEngine.iterate: identical bits in fixed-step mode; in adaptive mode up to the order in
// which the ranks' sums are added (rank order here, the collective's order there; two ranks: identical).
int iterate_peer(pdlp_handle h, int iters, int adaptive)
{
    int rc = PDLP_OK;
    pdlp_solver::Peer& P = h->peer;
    if (h->delta && iters > 0 && !h->carry.anchors_valid) return PDLP_ERR_STATE;       // (the caller refreshes the anchors: that needs gathers)
    if (iters == 0) return PDLP_OK;
    // entry handshake: a peer's first block may only arrive once this rank's stream has reached the iterations -- whatever this rank
    // did with its vectors before (a restart check, a restart) is behind the flag
    if ((rc = peer_signal(h, false)) != PDLP_OK || (rc = peer_wait(h)) != PDLP_OK) return rc;
    const bool saved_inline = h->begin_inline;
    h->begin_inline = true;                       // (the own-block panels go onto the handle's stream)
    // push form: the epilogues store locally; a copy kernel on the side stream carries the block to the peers while the handle's
    // stream multiplies the own block's panels -- where those panels are a good part of the product (2, 4 ranks) they hide the
    // transfer, which the stores of an epilogue, issued in the last microseconds of a half-step on the same stream, cannot
    const bool push = P.push;
    const bool first = P.local_first || push;
    P.active = !push;
    for (int it = 0; it < iters && rc == PDLP_OK; ++it) {
        if ((rc = pdlp_primal_half(h, adaptive)) != PDLP_OK) break;              // stores xbar (x+ - x) into the peers
        if ((rc = push ? peer_push_and_signal(h, h->delta ? 4 : 0, false) : peer_signal(h, false)) != PDLP_OK) break;
        if (first && (rc = pdlp_dual_half_begin(h, adaptive)) != PDLP_OK) break;              // K's panels over the own block of xbar
        if ((rc = peer_wait(h)) != PDLP_OK) break;
        if ((rc = pdlp_dual_half(h, adaptive)) != PDLP_OK) break;                // stores the new y (y+ - y) into the peers
        // (adaptive: this rank's three sums travel with the flag; the new y is in the buffer that has just become current)
        if ((rc = push ? peer_push_and_signal(h, h->delta ? 5 : 1 + h->ix_cur, adaptive != 0) : peer_signal(h, adaptive != 0)) != PDLP_OK) break;
        if (first && it + 1 < iters && (rc = pdlp_primal_half_begin(h)) != PDLP_OK) break;
        if ((rc = peer_wait(h, adaptive != 0)) != PDLP_OK) break;                // (adaptive: and the rule from all ranks' sums)
    }
    P.active = false;
    h->begin_inline = saved_inline;
    if (rc != PDLP_OK) return rc;
    HIP_TRY(hipGetLastError());
    if (!adaptive) return pdlp_fixed_advance(h, iters);
    return PDLP_OK;
}

// what a rank tells the others (pdlp_peer_export): PDLP_PEER_INFO_BYTES opaque bytes
struct PeerInfo {
    uint32_t magic, version;
    hipIpcMemHandle_t ws, box;
    int64_t ws_off;                 // the workspace inside its allocation (an IPC handle opens at the allocation's base)
    int64_t vec_off[6];             // xbar, the three y buffers, gdx, gdy inside the workspace
    int64_t n, m, nl, ml;
    int32_t dtype, pid;
    int64_t alloc_bytes;            // size of the allocation the workspace lies in (what a peer maps)
};
static_assert(sizeof(PeerInfo) <= PDLP_PEER_INFO_BYTES, "PeerInfo must fit its published size");
constexpr uint32_t PEER_MAGIC = 0x50444c50u;

void peer_vec_offsets(pdlp_handle h, int64_t off[6])
{
    off[0] = h->xbar - h->ws;
    for (int i = 0; i < 3; ++i) off[1 + i] = h->yb[i] - h->ws;
    off[4] = (char*)h->gdx - h->ws;
    off[5] = (char*)h->gdy - h->ws;
}

int peer_own_resources(pdlp_handle h)
{
    pdlp_solver::Peer& P = h->peer;
    if (!P.box) {
        HIP_TRY(hipExtMallocWithFlags((void**)&P.box, BOX_BYTES, hipDeviceMallocFinegrained));
        HIP_TRY(hipMemsetAsync(P.box, 0, BOX_BYTES, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    if (!P.err) {
        HIP_TRY(hipHostMalloc((void**)&P.err, 64, hipHostMallocMapped));
        *P.err = 0;
        HIP_TRY(hipHostGetDevicePointer((void**)&P.err_dev, P.err, 0));
    }
    return PDLP_OK;
}

}  // namespace

extern "C" {

int pdlp_peer_export(pdlp_handle h, void* info)
{
    if (!h || !info) return PDLP_ERR_INVALID;
    if (whole_problem(h)) return PDLP_ERR_STATE;              // not sharded: nothing to exchange
    HIP_TRY(hipSetDevice(h->p.device));
    int rc;
    if ((rc = peer_own_resources(h)) != PDLP_OK) return rc;
    PeerInfo pi{};
    pi.magic = PEER_MAGIC; pi.version = (uint32_t)pdlp_abi_version();
    hipDeviceptr_t base = nullptr;
    size_t range = 0;
    HIP_TRY(hipMemGetAddressRange(&base, &range, (hipDeviceptr_t)h->ws));
    if ((char*)h->ws + h->ws_bytes > (char*)base + range) return PDLP_ERR_WORKSPACE;   // (a workspace spanning allocations cannot be exported)
    // ROCm 7.2: hipIpcOpenMemHandle never returns for an allocation whose size has bit 31 set (2000 / 5000 MB open at once, 3000 /
    // 3826 / 4000 / 6500 MB hang, 4096 / 8192 / 9000 MB open: tools/ipc_torch_probe.py).  Refuse here rather than let a peer hang.
    if (range & 0x80000000ull) return PDLP_ERR_WORKSPACE;
    HIP_TRY(hipIpcGetMemHandle(&pi.ws, (void*)base));
    HIP_TRY(hipIpcGetMemHandle(&pi.box, (void*)h->peer.box));
    pi.ws_off = h->ws - (char*)base;
    peer_vec_offsets(h, pi.vec_off);
    pi.n = h->p.n; pi.m = h->p.m; pi.nl = h->nl; pi.ml = h->ml;
    pi.dtype = h->p.dtype; pi.pid = (int32_t)getpid();
    pi.alloc_bytes = (int64_t)range;
    std::memset(info, 0, PDLP_PEER_INFO_BYTES);
    std::memcpy(info, &pi, sizeof pi);
    return PDLP_OK;
}

int pdlp_peer_connect(pdlp_handle h, int rank, int world, const void* infos, int flags)
{
    if (!h || world < 2 || world > MAX_PEER + 1 || rank < 0 || rank >= world) return PDLP_ERR_INVALID;
    if (h->nl * world != h->p.n || h->ml * world != h->p.m || h->p.col0 != (int64_t)rank * h->nl || h->p.row0 != (int64_t)rank * h->ml)
        return PDLP_ERR_INVALID;                   // equal blocks, this rank's at rank * block (torchpdlp_amd/distributed.py)
    if (has_extension(h)) return PDLP_ERR_STATE;      // (two-sided rows and the quadratic term have no sharded form)
    const bool loopback = (flags & PDLP_PEER_LOOPBACK) != 0;
    if (!loopback && !infos) return PDLP_ERR_INVALID;
    HIP_TRY(hipSetDevice(h->p.device));
    pdlp_solver::Peer& P = h->peer;
    if (P.on) return PDLP_ERR_STATE;
    int rc;
    if ((rc = peer_own_resources(h)) != PDLP_OK) return rc;
    P.rank = rank; P.world = world; P.n = 0; P.loopback = loopback;
    if (loopback) {
        // timing stand-in (tools/shard_iter_timing.py): rank `rank` of `world` alone -- every "peer vector" is a scratch block of this
        // process, every flag lands in the own mailbox (the waits pass at once).  What it prices: the stores and the two launches.
        const size_t blk = (size_t)(h->nl > h->ml ? h->nl : h->ml) * 8;
        HIP_TRY(hipMalloc((void**)&P.scratch, blk * (size_t)(world - 1)));
        char* slow = nullptr;
        if (flags & PDLP_PEER_LOOPBACK_HOST) {
            // the first "peer" lives in pinned host memory: its block crosses PCIe (~55 GB/s: 5 MB in ~0.09 ms), about what the seven
            // blocks of an 8-rank exchange take over xGMI together -- so the loopback also shows how much of a slow drain of the
            // stores a schedule hides
            HIP_TRY(hipHostMalloc((void**)&P.scratch_host, blk, hipHostMallocMapped));
            HIP_TRY(hipHostGetDevicePointer((void**)&slow, P.scratch_host, 0));
        }
        for (int q = 0, i = 0; q < world; ++q) {
            if (q == rank) continue;
            for (int v = 0; v < 6; ++v) P.out[v][i] = (i == 0 && slow) ? slow : P.scratch + blk * (size_t)i;
            P.flag[i] = (uint32_t*)P.box + (size_t)q * BOX_FLAG_STRIDE;
            P.sums[i] = (double*)(P.box + BOX_BYTES / 2) + (size_t)q * BOX_SUMS_STRIDE;     // (an unused part of the mailbox: the peers' slots stay zero)
            ++i;
            P.n = i;
        }
        P.on = true;
        return PDLP_OK;
    }
    int64_t mine[6];
    peer_vec_offsets(h, mine);
    for (int q = 0, i = 0; q < world; ++q) {
        if (q == rank) continue;
        PeerInfo pi;
        std::memcpy(&pi, (const char*)infos + (size_t)q * PDLP_PEER_INFO_BYTES, sizeof pi);
        if (pi.magic != PEER_MAGIC || pi.version != (uint32_t)pdlp_abi_version() || pi.n != h->p.n || pi.m != h->p.m || pi.nl != h->nl ||
            pi.ml != h->ml || pi.dtype != h->p.dtype) { peer_release(h); return PDLP_ERR_INVALID; }
        char *wsb = nullptr, *box = nullptr;
        if (hipIpcOpenMemHandle((void**)&wsb, pi.ws, hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); peer_release(h); return PDLP_ERR_COMM; }
        P.opened[P.nopened++] = wsb;
        if (hipIpcOpenMemHandle((void**)&box, pi.box, hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); peer_release(h); return PDLP_ERR_COMM; }
        P.opened[P.nopened++] = box;
        for (int v = 0; v < 6; ++v) P.out[v][i] = wsb + pi.ws_off + pi.vec_off[v] + peer_block_start(h, v);
        P.flag[i] = (uint32_t*)box + (size_t)rank * BOX_FLAG_STRIDE;
        P.sums[i] = (double*)(box + BOX_SUMS_AT) + (size_t)rank * BOX_SUMS_STRIDE;
        ++i;
        P.n = i;
    }
    P.on = true;
    return PDLP_OK;
}

int pdlp_peer_status(pdlp_handle h, int32_t out[4])
{
    if (!h || !out) return PDLP_ERR_INVALID;
    out[0] = h->peer.on; out[1] = h->peer.enabled;
    out[2] = h->peer.err ? __atomic_load_n(h->peer.err, __ATOMIC_RELAXED) : 0;
    out[3] = (int32_t)h->peer.seq;
    return PDLP_OK;
}

int pdlp_peer_close(pdlp_handle h)
{
    if (!h) return PDLP_ERR_INVALID;
    (void)hipStreamSynchronize(h->stream);
    peer_release(h);
    return PDLP_OK;
}

}  // extern "C"
