// pdlp_hip.hip -- restarted PDHG for LP on AMD Instinct MI355X (gfx950, wave64), C ABI in include/pdlp_hip.h.
//
// The library is ONE translation unit: this file holds the constants, the wave helpers and the entry points of the ABI, and
// includes everything else (DESIGN.md has the long form of the design).  In the order of inclusion -- a file may use what the
// files before it define:
//   kernels (inside this file's anonymous namespace)
//     pdlp_epilogues.inc      the functors a product's epilogue runs per row: half-steps, KKT sums, report, delta mode, stores
//     pdlp_kernel_csr.inc     k_csr_fused / k_long_rows: the CSR row-block product
//     pdlp_kernel_tiled.inc   k_tiled_fused, k_rowsum_epilogue, the remainder kernels: the panel-tiled product
//     pdlp_kernels_small.inc  vector kernels, the step-size rule, the direct exchange's signal / wait, Ruiz, probes
//     pdlp_kernel_mv.inc      population kernels (many vectors per product)
//     pdlp_kernel_batch.inc   batched solves
//   host side (at file scope; each opens its own anonymous namespace and, where it has entry points, its own extern "C" block)
//     pdlp_loaders.inc        RCCL and roctx resolved with dlopen, Range; pdlp_trace_enable / pdlp_range_*
//     pdlp_handle.inc         Schedule, Carried (which carried product still belongs to its vector: the rules and the only writers),
//                             struct pdlp_solver, the workspace Layout and its capacities, check / bind / free
//     pdlp_schedule.inc       row-block and long-row schedules built on the host (K, K' and the objective's Q), the split-product
//                             planner (configure_split)
//     pdlp_products.inc       launch_mat and what it is made of, the products with Q, the shared launch helpers, the half-steps
//     pdlp_delta.inc          delta mode (mixed precision): half-steps and KKT from anchors; pdlp_set_delta / _anchors / _state
//     pdlp_kkt.inc            KKT pass, report, flush / average / distance / infeasibility / power iteration; pdlp_restart
//     pdlp_population.inc     the mv_* launchers; pdlp_mv_combine
//     pdlp_driver.inc         the library's iteration driver: direct, graph replay, sharded over RCCL; pdlp_comm_*
//     pdlp_halpern.inc        the reflected Halpern iteration (opt-in solve mode); pdlp_halpern_iterate, pdlp_halpern_fixed_point
//     pdlp_peer.inc           the direct exchange over HIP IPC: iterate_peer; pdlp_peer_*
//     pdlp_ruiz.inc           entry points that take no handle: Ruiz blocks, pdlp_vec_*, the bandwidth probes
//     pdlp_batch_host.inc     batched solves: launch shapes and pdlp_batch_*
// Where an entry point lives: one that is argument checks plus one call (or a few assignments to the handle's flags) is HERE, so
// that this file reads as the table of contents of the ABI; one whose body IS its subsystem's logic is in an extern "C" block at the
// end of that subsystem's file (named in the list above).
// This bandwidth-bound path uses no MFMA.  Written for gfx950 only.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>      // types and prototypes only: the library is resolved with dlopen when a communicator is asked for
#include <dlfcn.h>
#include <unistd.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "pdlp_hip.h"

namespace {

constexpr int BLOCK = 256;       // threads per workgroup (4 wave64)
constexpr int NNZ_CAP = 2048;    // non-zeros staged in LDS per row block
constexpr int ROWS_CAP = 256;    // rows per row block (one epilogue lane each at most)
constexpr int MAX_GRID = 2048;   // 256 CUs x 8 workgroups
constexpr int NACC = 4;          // partial sums a kernel may produce
constexpr int MAX_CHUNKS = 4;    // chunks of the exchange of a gathered vector (sharded problems)
constexpr int MAX_PHASE = MAX_CHUNKS + 2;
constexpr int MAX_PEER = 7;      // direct exchange (pdlp_peer_*): the other ranks of one node
constexpr int PEER_WAIT_BLOCKS = 8; // one waiting wave per XCD (k_peer_wait)
// a rank's mailbox for the direct exchange (fine-grained device memory, opened by every peer): the sequence number rank q last
// signalled, one per 64-byte line, then rank q's three sums of the step-size rule
constexpr int BOX_BYTES = 4096, BOX_FLAG_STRIDE = 16 /* uint32 */, BOX_SUMS_AT = 1024 /* bytes */, BOX_SUMS_STRIDE = 4 /* doubles */;

// indices into the device scalar block (double[PDLP_NSCAL])
enum { S_ETA = 0, S_OMEGA, S_THETA, S_TAU, S_SIGMA, S_WPEND, S_ETASUM, S_K, S_INV1PT, S_ACCEPT, S_ETABAR, S_DEN, S_ETASUM_PREV, S_CURV };

#define HIP_TRY(expr)                                                   \
    do {                                                                \
        hipError_t e_ = (expr);                                         \
        if (e_ != hipSuccess) return PDLP_ERR_HIP_BASE - (int)e_;       \
    } while (0)

template <typename T> __device__ __forceinline__ T shfl_xor_t(T v, int m) { return __shfl_xor(v, m, 64); }

// sum of `v` over the 256-thread workgroup, valid in thread 0.  `buf` holds >= 4 entries.
// inclusive scan over the 64 lanes of a wave with DPP adds only (no LDS crossbar): Hillis-Steele inside each row of
// 16 lanes, then row_bcast:15 / row_bcast:31 carry the row totals.  All 64 lanes must be active.
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t x)
{
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);   // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);   // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);   // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);   // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return x;
}

// two independent inclusive scans at once, written out: the compiler fuses the DPP move into the add for one scan of such
// a pair but not reliably for the other (18 instead of 6 VALU instructions).  A DPP read of a VGPR needs 2 wait states after
// the VALU write of it: the other scan's instruction and one s_nop provide them.
__device__ __forceinline__ void wave_incl_scan2_u32(uint32_t& a, uint32_t& b)
{
#define PDLP_SCAN_STEP(ctl) "v_add_u32_dpp %0, %0, %0 " ctl "\n\tv_add_u32_dpp %1, %1, %1 " ctl "\n\ts_nop 0\n\t"
    asm("s_nop 1\n\t"
        PDLP_SCAN_STEP("row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        PDLP_SCAN_STEP("row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        PDLP_SCAN_STEP("row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        PDLP_SCAN_STEP("row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        PDLP_SCAN_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf")
        PDLP_SCAN_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")
        : "+v"(a), "+v"(b));
#undef PDLP_SCAN_STEP
}

template <typename T> __device__ __forceinline__ T block_sum(T v, T* buf)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += shfl_xor_t(v, off);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) buf[w] = v;
    __syncthreads();
    return buf[0] + buf[1] + buf[2] + buf[3];
}

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
inline int grid_for(int64_t n) { int64_t g = (n + BLOCK - 1) / BLOCK; return (int)(g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g)); }
inline int rows_grid(int64_t rows) { return rows > 0 ? grid_for(rows) : 0; }      // (no rows: no launch, no partial sums)

// a function template in the handle's working precision (float64 vectors in mixed precision) ...
#define DISPATCH(h, fn, ...) ((h)->p.dtype == PDLP_F32 ? fn<float>(__VA_ARGS__) : fn<double>(__VA_ARGS__))
// ... and a statement (one kernel launch) that sees the element type a PDLP_F32 / PDLP_F64 / PDLP_MIXED code names as T
#define WITH_T(dtype, ...)                                              \
    do {                                                                \
        if ((dtype) == PDLP_F32) { using T = float; __VA_ARGS__; }      \
        else { using T = double; __VA_ARGS__; }                         \
    } while (0)

#include "pdlp_epilogues.inc"
#include "pdlp_kernel_csr.inc"
#include "pdlp_kernel_tiled.inc"
#include "pdlp_kernels_small.inc"
#include "pdlp_kernel_mv.inc"
#include "pdlp_kernel_batch.inc"

}  // namespace

#include "pdlp_loaders.inc"
#include "pdlp_handle.inc"
#include "pdlp_schedule.inc"
#include "pdlp_products.inc"
#include "pdlp_delta.inc"
#include "pdlp_kkt.inc"
#include "pdlp_population.inc"
#include "pdlp_driver.inc"
#include "pdlp_halpern.inc"
#include "pdlp_peer.inc"
#include "pdlp_ruiz.inc"

// ================================================================================================
// C ABI: the entry points that are argument checks plus one call (the others: see the map at the top)
// ================================================================================================
extern "C" {

// 18: pdlp_batch_* (batched solves over one matrix); pdlp_batch_attach_matrices, pdlp_batch_product, pdlp_halpern_iterate, then
//     pdlp_pack_tile_items / pdlp_attach_packed_items (7-byte items on the float32 path; struct pdlp_tiles is unchanged),
//     pdlp_halpern_fixed_point, the pdlp_*objective_matrix* calls and pdlp_objective_iterate joined them without a change to any
//     existing signature or struct, so the number stands
// 17: pdlp_peer_* (direct exchange over HIP IPC), PDLP_OPT_BEGIN_INLINE
// 16: pdlp_set_option (the library reads no environment variables), pdlp_mv_product, pdlp_mv_combine, pdlp_vec_sqdist,
//     pdlp_probe_gather, pdlp_tile_limits reports the threads per workgroup, pdlp_primal_half_piece / pdlp_dual_half_piece (results
//     of split products leave piece by piece), pdlp_trace_enable / pdlp_range_push / pdlp_range_pop (roctx), pdlp_adaptive_retry
// 15: 64-bit row pointers, row-block bases of the tiles and schedule offsets (more than 2^31 non-zeros per handle)
// 14: pdlp_probe_stream_read
// 13: chunked exchange (pdlp_set_exchange_chunks, pdlp_exchange_plan, pdlp_half_chunk)
// 12: count words of a tile laid out for coalesced loads
// 11: pdlp_comm_load
// 10: pdlp_set_anchors
//  9: pdlp_attach_sorted
//  8: running products, pdlp_flush_average(h, adaptive)
//  7: pdlp_comm_*
//  6: remainder of a tiled matrix
//  5: PDLP_MIXED, delta mode
//  4: pdlp_tile_limits, pdlp_csr_div_cols takes nnz
int pdlp_abi_version(void) { return 18; }

const char* pdlp_strerror(int code)
{
    switch (code) {
        case PDLP_OK: return "ok";
        case PDLP_ERR_INVALID: return "invalid argument";
        case PDLP_ERR_WORKSPACE: return "workspace too small or not 256-byte aligned";
        case PDLP_ERR_STATE: return "call sequence violated";
        case PDLP_ERR_COMM:
            return g_rccl.GetErrorString && g_rccl.last_error ? g_rccl.GetErrorString((ncclResult_t)g_rccl.last_error)
                                                              : "RCCL could not be loaded or a collective failed";
        default: break;
    }
    if (code <= PDLP_ERR_HIP_BASE) return hipGetErrorString((hipError_t)(PDLP_ERR_HIP_BASE - code));
    return "unknown error";
}

int pdlp_workspace_bytes(const pdlp_problem* p, int64_t* bytes)
{
    int rc = check_problem(p);
    if (rc != PDLP_OK || !bytes) return PDLP_ERR_INVALID;
    HIP_TRY(hipSetDevice(p->device));
    int64_t nnzK = 0, nnzKT = 0;
    if ((rc = read_last_rowptr(p->K_rowptr, p->row1 - p->row0, &nnzK, (hipStream_t)p->stream)) != PDLP_OK) return rc;
    if ((rc = read_last_rowptr(p->KT_rowptr, p->col1 - p->col0, &nnzKT, (hipStream_t)p->stream)) != PDLP_OK) return rc;
    *bytes = layout(p, nnzK, nnzKT).bytes;
    return PDLP_OK;
}

int pdlp_create(pdlp_handle* out, const pdlp_problem* p, void* workspace, int64_t workspace_bytes)
{
    int rc = check_problem(p);
    if (rc != PDLP_OK || !out) return PDLP_ERR_INVALID;
    HIP_TRY(hipSetDevice(p->device));
    const int64_t nl = p->col1 - p->col0, ml = p->row1 - p->row0;
    std::vector<int64_t> rpK((size_t)ml + 1, 0), rpKT((size_t)nl + 1, 0);
    hipStream_t pstream = (hipStream_t)p->stream;
    if (ml > 0) HIP_TRY(hipMemcpyAsync(rpK.data(), p->K_rowptr, (size_t)(ml + 1) * 8, hipMemcpyDeviceToHost, pstream));
    if (nl > 0) HIP_TRY(hipMemcpyAsync(rpKT.data(), p->KT_rowptr, (size_t)(nl + 1) * 8, hipMemcpyDeviceToHost, pstream));
    HIP_TRY(hipStreamSynchronize(pstream));     // (ordered behind whatever produced the arrays on that stream)
    if (rpK[0] != 0 || rpKT[0] != 0) return PDLP_ERR_INVALID;
    const Layout L = layout(p, rpK[ml], rpKT[nl]);
    if (!workspace || workspace_bytes < L.bytes || ((uintptr_t)workspace & 255u)) return PDLP_ERR_WORKSPACE;

    pdlp_solver* h = new (std::nothrow) pdlp_solver();
    if (!h) return PDLP_ERR_INVALID;
    // what depends on the problem; every other field keeps the initialiser of its declaration (pdlp_handle.inc)
    h->p = *p;
    h->stream = (hipStream_t)p->stream;
    h->es = p->dtype == PDLP_F32 ? 4 : 8;
    h->mixed = p->dtype == PDLP_MIXED;
    h->nl = nl;
    h->ml = ml;
    h->nnz = rpK[ml];
    int64_t ie = p->m_ineq - p->row0;
    h->ineq_end = (int)(ie < 0 ? 0 : (ie > ml ? ml : ie));
    bind_layout(h, (char*)workspace, L);
    open_side_stream(h);
    if ((rc = upload_schedules(h, rpK, rpKT)) != PDLP_OK) { free_handle(h); return rc; }
    // Zero every state vector, scratch and scalar: [xb[0], sched[0]) and [dxf, rplo[0]).  NOT zeroed: the schedules, the long-row
    // tables and the row pointers' low words -- upload_schedules has just filled them -- and the row-sum scratch between them
    // (written by every product before it is read).
    char* w = h->ws;
    if (hipMemsetAsync(w + L.xb[0], 0, (size_t)(L.sched[0] - L.xb[0]), h->stream) != hipSuccess ||
        hipMemsetAsync(w + L.dxf, 0, (size_t)(L.rplo[0] - L.dxf), h->stream) != hipSuccess) { free_handle(h); return PDLP_ERR_HIP_BASE - 1; }
    WITH_T(p->dtype, hipLaunchKernelGGL(k_set_step<T>, dim3(1), dim3(1), 0, h->stream, h->sc, 0.0, 1.0, 1.0, 0.0));
    *out = h;
    return PDLP_OK;
}

void pdlp_destroy(pdlp_handle h)
{
    if (!h) return;
    (void)hipStreamSynchronize(h->stream);
    free_handle(h);
}

int pdlp_buffer_ptr(pdlp_handle h, int which, void** ptr)
{
    if (!h || !ptr) return PDLP_ERR_INVALID;
    switch (which) {
        case PDLP_BUF_X_CUR: *ptr = h->xb[h->ix_cur]; break;
        case PDLP_BUF_X_PREV: *ptr = h->xb[h->ix_prev]; break;
        case PDLP_BUF_XBAR: *ptr = h->xbar; break;
        case PDLP_BUF_X_AVG: *ptr = h->xb[h->ix_avg]; break;
        case PDLP_BUF_Y_CUR: *ptr = h->yb[h->ix_cur]; break;
        case PDLP_BUF_Y_PREV: *ptr = h->yb[h->ix_prev]; break;
        case PDLP_BUF_Y_AVG: *ptr = h->yb[h->ix_avg]; break;
        case PDLP_BUF_RED: *ptr = h->red; break;
        case PDLP_BUF_X_SUM: *ptr = h->x_sum; break;
        case PDLP_BUF_Y_SUM: *ptr = h->y_sum; break;
        case PDLP_BUF_SCALARS: *ptr = h->sc; break;
        case PDLP_BUF_DX: *ptr = h->dxf; break;
        case PDLP_BUF_DY: *ptr = h->dyf; break;
        case PDLP_BUF_LAM_PREV: *ptr = h->lam_prev; break;
        case PDLP_BUF_GDX: if (!h->mixed) return PDLP_ERR_STATE; *ptr = h->gdx; break;
        case PDLP_BUF_GDY: if (!h->mixed) return PDLP_ERR_STATE; *ptr = h->gdy; break;
        default: return PDLP_ERR_INVALID;
    }
    return PDLP_OK;
}

int pdlp_attach_tiles(pdlp_handle h, int transpose, const pdlp_tiles* t)
{
    if (!h) return PDLP_ERR_INVALID;
    Schedule& s = transpose ? h->sKT : h->sK;
    drop_graphs(h);               // captured launches name the old kernel and arrays
    s.idx24 = s.run_base = nullptr;      // (a packed index stream belongs to the tile set it was made from: attach it again)
    if (!t) { s.tiled = false; return configure_split(h, transpose != 0); }
    const int64_t rows = transpose ? h->nl : h->ml;
    const int rpt_max = h->p.dtype == PDLP_F64 ? TileCfg<double, double>::RPT_MAX : TileCfg<float, float>::RPT_MAX;   // (mixed: float32 tiles)
    const int cap_max = h->p.dtype == PDLP_F64 ? TileCfg<double, double>::CAP : TileCfg<float, float>::CAP;
    if (t->rpt < 1 || t->rpt > rpt_max || t->cap > cap_max || t->lw < 4 || (((uint64_t)t->cap + 8u) << t->lw) > (1ull << 32)) return PDLP_ERR_INVALID;   // (slot, column) must pack into 32 bits
    const int64_t rb = (int64_t)TNT * t->rpt;
    if (t->nblk != (int)((rows + rb - 1) / rb) || t->npanel < 1) return PDLP_ERR_INVALID;
    if (t->groups < 1 || t->groups > h->rs_groups || t->groups > t->npanel) return PDLP_ERR_INVALID;
    if (t->nblk > h->part_blocks) return PDLP_ERR_INVALID;             // one slot of partial sums per workgroup
    // (every group owns at least one panel: the kernel splits the panels evenly, groups <= npanel was checked above)
    if (!t->idx || !t->val || !t->tile_ptr || !t->blk_base || !t->cnt) return PDLP_ERR_INVALID;
    if (((uintptr_t)t->idx & 15u) || ((uintptr_t)t->val & 15u) || ((uintptr_t)t->cnt & 15u)) return PDLP_ERR_INVALID;
    if (t->rem_rows_n < 0 || t->rem_segs_n < t->rem_rows_n) return PDLP_ERR_INVALID;
    if (t->rem_rows_n > 0 && (!t->rem_rows || !t->rem_rptr || !t->rem_sptr || !t->rem_col || !t->rem_val || !t->rem_work || !t->rem_extra ||
                              (h->mixed && !t->rem_extra_f32)))
        return PDLP_ERR_INVALID;
    s.t = *t;
    s.tiled = true;
    return configure_split(h, transpose != 0);
}

int pdlp_pack_tile_items(const uint32_t* idx, int64_t items, int lw, uint32_t* idx24, uint32_t* run_base, int32_t* flag, void* stream)
{
    if (!idx || !idx24 || !run_base || !flag || items < 0 || (items & 255) || lw < 4 || lw > 16) return PDLP_ERR_INVALID;      // (a run base is 16 bits)
    if (((uintptr_t)idx & 15u) || ((uintptr_t)idx24 & 3u) || ((uintptr_t)run_base & 3u) || ((uintptr_t)flag & 3u)) return PDLP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nchunks = items >> 8;
    HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(run_base + nchunks * 2, 0, (size_t)P24_BASE_TAIL * 8, st));      // the spare entries behind the last chunk
    if (nchunks > 0) {
        hipLaunchKernelGGL(k_pack_items24, dim3(grid_for(nchunks * 64)), dim3(BLOCK), 0, st, idx, nchunks, lw, idx24, run_base, flag);
        HIP_TRY(hipGetLastError());
    }
    return PDLP_OK;
}

int pdlp_attach_packed_items(pdlp_handle h, int transpose, const uint32_t* idx24, const uint32_t* run_base)
{
    if (!h || (idx24 == nullptr) != (run_base == nullptr)) return PDLP_ERR_INVALID;
    Schedule& s = transpose ? h->sKT : h->sK;
    if (idx24) {
        if (!s.tiled || h->p.dtype != PDLP_F32) return PDLP_ERR_STATE;      // float32 handles with tiles attached
        if (s.t.cap > (1 << P24_SLOT_BITS) || s.t.lw > 16 || ((uintptr_t)idx24 & 3u) || ((uintptr_t)run_base & 3u)) return PDLP_ERR_INVALID;
    }
    if (s.pending) return PDLP_ERR_STATE;        // not in the middle of a split product
    drop_graphs(h);               // captured launches name the other kernel
    s.idx24 = idx24;
    s.run_base = run_base;
    return PDLP_OK;
}

int pdlp_schedule_info(pdlp_handle h, int transpose, int32_t* nblk, const int64_t** blocks)
{
    if (!h || !nblk || !blocks) return PDLP_ERR_INVALID;
    const Schedule& s = transpose ? h->sKT : h->sK;
    *nblk = s.nblk;
    *blocks = s.blk;
    return PDLP_OK;
}

int pdlp_attach_sorted(pdlp_handle h, int transpose, const uint32_t* sidx, const void* sval, const int32_t* cbase)
{
    if (!h) return PDLP_ERR_INVALID;
    if ((sidx == nullptr) != (sval == nullptr) || (sidx == nullptr) != (cbase == nullptr)) return PDLP_ERR_INVALID;
    Schedule& s = transpose ? h->sKT : h->sK;
    drop_graphs(h);
    s.sidx = sidx; s.sval = sval; s.cbase = cbase;
    return PDLP_OK;
}

int pdlp_set_iterate(pdlp_handle h, const void* x_local, const void* y_local)
{
    if (!h || !x_local || !y_local) return PDLP_ERR_INVALID;
    HIP_TRY(hipMemcpyAsync(h->xb[h->ix_cur] + h->p.col0 * h->es, x_local, h->nl * h->es, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->yb[h->ix_cur] + h->p.row0 * h->es, y_local, h->ml * h->es, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->x_last, x_local, h->nl * h->es, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->y_last, y_local, h->ml * h->es, hipMemcpyDeviceToDevice, h->stream));
    int rc = zero_sums(h, true);
    if (rc == PDLP_OK) h->carry.new_iterate();
    return rc;
}

// q_upper (two-sided rows) or d (quadratic term) set, replaced or taken away.  The forms without them: mixed precision / delta mode,
// a shard of a problem, an exchange of any kind.  (This is also what keeps pdlp_set_delta(on) away from d: it asks for a PDLP_MIXED
// handle, which can never have it set.)
static int set_operand(pdlp_handle h, const void* pdlp_solver::*operand, const void* local)
{
    if (!h) return PDLP_ERR_INVALID;
    if (local && !plain_single(h)) return PDLP_ERR_STATE;
    if (mid_split_product(h)) return PDLP_ERR_STATE;
    drop_graphs(h);               // captured launches hold the functors without (or with the old) operand
    h->*operand = local;
    h->carry.operands_changed();
    return PDLP_OK;
}

int pdlp_set_row_upper(pdlp_handle h, const void* q_upper_local) { return set_operand(h, &pdlp_solver::q_upper, q_upper_local); }
int pdlp_set_objective_diag(pdlp_handle h, const void* d_local) { return set_operand(h, &pdlp_solver::obj_diag, d_local); }

int pdlp_objective_matrix_bytes(pdlp_handle h, int64_t nnz, int64_t* bytes)
{
    if (!h || !bytes || nnz < 0) return PDLP_ERR_INVALID;
    *bytes = objective_matrix_layout(h->p.n, nnz, (int64_t)h->es).bytes;
    return PDLP_OK;
}

// Q set, replaced or taken away (NULL arrays).  The forms without it are those without the other extensions (set_operand), and graph
// replay: a captured pair would have to hold the gradient product, which PDLP_OPT_GRAPH refuses while Q is set.
int pdlp_set_objective_matrix(pdlp_handle h, const int64_t* rowptr, const int32_t* colidx, const void* val, void* work, int64_t work_bytes)
{
    if (!h) return PDLP_ERR_INVALID;
    const bool on = rowptr || colidx || val;
    if (on && (!rowptr || !colidx || !val)) return PDLP_ERR_INVALID;
    if (on && (!plain_single(h) || h->graph_ok)) return PDLP_ERR_STATE;
    if (mid_split_product(h)) return PDLP_ERR_STATE;
    if (on) {
        const int64_t n = h->p.n;
        std::vector<int64_t> rp((size_t)n + 1, 0);
        HIP_TRY(hipMemcpyAsync(rp.data(), rowptr, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));     // (ordered behind whatever produced the arrays on that stream)
        if (rp[0] != 0) return PDLP_ERR_INVALID;
        for (int64_t r = 0; r < n; ++r) if (rp[(size_t)r + 1] < rp[(size_t)r]) return PDLP_ERR_INVALID;
        if (!work || work_bytes < objective_matrix_layout(n, rp[(size_t)n], (int64_t)h->es).bytes || ((uintptr_t)work & 255u)) return PDLP_ERR_WORKSPACE;
        const int rc = upload_objective_schedule(h, rp, (char*)work);
        if (rc != PDLP_OK) return rc;
    } else {
        h->sQ = Schedule();
        h->obj_mat.part = nullptr;
    }
    drop_graphs(h);
    h->obj_mat.on = on;
    h->obj_mat.colidx = colidx;
    h->obj_mat.val = val;
    h->carry.objective_matrix_changed();
    return PDLP_OK;
}

int pdlp_objective_product(pdlp_handle h, const void* x_full, void* out_local)
{
    if (!h || !x_full || !out_local) return PDLP_ERR_INVALID;
    if (!h->obj_mat.on) return PDLP_ERR_STATE;
    return DISPATCH(h, obj_product_t, h, x_full, out_local);
}

int pdlp_get_iterate(pdlp_handle h, int which, void* x_local, void* y_local)
{
    if (!h) return PDLP_ERR_INVALID;
    const int ix = iterate_index(h, which);
    if (ix < 0) return PDLP_ERR_INVALID;
    if (x_local) HIP_TRY(hipMemcpyAsync(x_local, h->xb[ix] + h->p.col0 * h->es, h->nl * h->es, hipMemcpyDeviceToDevice, h->stream));
    if (y_local) HIP_TRY(hipMemcpyAsync(y_local, h->yb[ix] + h->p.row0 * h->es, h->ml * h->es, hipMemcpyDeviceToDevice, h->stream));
    return PDLP_OK;
}

int pdlp_set_step(pdlp_handle h, double eta, double omega, double theta, int64_t iteration)
{
    if (!h || !(omega > 0.0)) return PDLP_ERR_INVALID;
    WITH_T(h->p.dtype, hipLaunchKernelGGL(k_set_step<T>, dim3(1), dim3(1), 0, h->stream, h->sc, eta, omega, theta, (double)iteration));
    HIP_TRY(hipGetLastError());
    // inside an averaging period a new eta ends the running products: the fixed step adds K'y of an iterate to its running sum with
    // the eta of the NEXT iteration (the product only exists then), y_sum has it with its own, so K'y_avg from the sums would not be
    // K' y_avg any more; the checks multiply until the next restart
    h->carry.sums_end();
    return PDLP_OK;
}

int pdlp_set_omega(pdlp_handle h, double omega)
{
    if (!h || !(omega > 0.0)) return PDLP_ERR_INVALID;
    WITH_T(h->p.dtype, hipLaunchKernelGGL(k_set_omega<T>, dim3(1), dim3(1), 0, h->stream, h->sc, omega));
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

int pdlp_get_scalars(pdlp_handle h, double out[PDLP_NSCAL])
{
    if (!h || !out) return PDLP_ERR_INVALID;
    HIP_TRY(hipMemcpyAsync(out, h->sc, PDLP_NSCAL * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PDLP_OK;
}

int pdlp_primal_half(pdlp_handle h, int adaptive)
{
    if (!h) return PDLP_ERR_INVALID;
    if (adaptive && h->obj_mat.on) return PDLP_ERR_STATE;      // (the linearised step of a sparse quadratic objective: fixed step only)
    h->carry.buffers_reassigned();
    if (h->delta) return delta_primal_half(h, adaptive);
    return DISPATCH(h, primal_half_t, h, adaptive);
}

int pdlp_dual_half(pdlp_handle h, int adaptive)
{
    if (!h) return PDLP_ERR_INVALID;
    if (adaptive && h->obj_mat.on) return PDLP_ERR_STATE;
    h->carry.buffers_reassigned();
    if (h->delta) return delta_dual_half(h, adaptive);
    return DISPATCH(h, dual_half_t, h, adaptive);
}

int pdlp_primal_half_piece(pdlp_handle h, int adaptive, int piece, int pieces) { return half_piece(h, false, adaptive, piece, pieces); }
int pdlp_dual_half_piece(pdlp_handle h, int adaptive, int piece, int pieces) { return half_piece(h, true, adaptive, piece, pieces); }

int pdlp_primal_half_begin(pdlp_handle h)
{
    if (!h) return PDLP_ERR_INVALID;
    if (h->delta && !h->carry.anchors_valid) return PDLP_OK;
    return DISPATCH(h, half_begin_t, h, true, h->yb[h->ix_cur]);
}

int pdlp_dual_half_begin(pdlp_handle h, int adaptive)
{
    if (!h) return PDLP_ERR_INVALID;
    if (h->delta && !h->carry.anchors_valid) return PDLP_OK;
    if (!h->delta && !h->carry.kx_valid) return PDLP_OK;        // the K x refresh ahead of this half-step uses the same scratch
    return DISPATCH(h, half_begin_t, h, false, h->xbar);
}

int pdlp_split_info(pdlp_handle h, int transpose, int32_t out[4])
{
    if (!h || !out) return PDLP_ERR_INVALID;
    const Schedule& s = transpose ? h->sKT : h->sK;
    out[0] = s.loc_pa; out[1] = s.loc_pb; out[2] = s.slotsA; out[3] = s.slotsB;
    return PDLP_OK;
}

int pdlp_set_option(pdlp_handle h, int option, int64_t value)
{
    if (!h) return PDLP_ERR_INVALID;
    if (mid_split_product(h)) return PDLP_ERR_STATE;
    switch (option) {
        case PDLP_OPT_RUNNING_KKT:
            // (switched back on inside a period: the running sums were not kept meanwhile -- no running average before the next restart)
            if (h->no_running && value != 0) h->carry.sums_end();
            h->no_running = value == 0;
            return PDLP_OK;
        case PDLP_OPT_KTY_REUSE: h->no_kty_reuse = value == 0; return PDLP_OK;
        case PDLP_OPT_GRAPH:
            if (value != 0 && h->obj_mat.on) return PDLP_ERR_STATE;      // (no replay with a sparse quadratic objective)
            drop_graphs(h);
            if (h->graph_ok) h->carry.sums_end();      // (nor while replay was on)
            h->graph_ok = value != 0 && h->side_ok && !h->comm;
            return (value != 0 && !h->graph_ok) ? PDLP_ERR_STATE : PDLP_OK;
        case PDLP_OPT_BEGIN_INLINE: h->begin_inline = value != 0; return PDLP_OK;
        case PDLP_OPT_PEER_EXCHANGE: h->peer.enabled = value != 0; return PDLP_OK;
        case PDLP_OPT_PEER_LOCAL_FIRST: h->peer.local_first = value != 0; return PDLP_OK;
        case PDLP_OPT_PEER_PUSH: h->peer.push = value != 0; return PDLP_OK;
        case PDLP_OPT_PEER_TIMEOUT_MS:
            if (value < 1 || value > 3600000) return PDLP_ERR_INVALID;
            h->peer.limit_ticks = (long long)value * 100000;            // (the wait kernel counts a 100 MHz clock)
            return PDLP_OK;
        case PDLP_OPT_PRODUCER_PIECES:
            h->producer_pieces = value != 0;
            return reconfigure_splits(h);
        case PDLP_OPT_SPLIT_SLOTS: {
            const int a = (int)(value & 0xffff), b = (int)((value >> 16) & 0xffff);
            if (value != 0 && (a < 1 || b < 1 || a + b > h->rs_groups)) return PDLP_ERR_INVALID;
            h->split_local = a;
            h->split_other = b;
            return reconfigure_splits(h);
        }
        default: return PDLP_ERR_INVALID;
    }
}

int pdlp_set_exchange_chunks(pdlp_handle h, int chunks)
{
    if (!h || chunks < 1 || chunks > MAX_CHUNKS) return PDLP_ERR_INVALID;
    if (mid_split_product(h)) return PDLP_ERR_STATE;
    h->xchunks = chunks;
    return reconfigure_splits(h);
}

int pdlp_exchange_plan(pdlp_handle h, int transpose, int32_t* nchunks, int64_t bounds[5])
{
    if (!h || !nchunks || !bounds) return PDLP_ERR_INVALID;
    // (a function of the block length and the requested count only: the same on every rank, whether or not this rank's own
    // product is split -- the pieces are collectives)
    int64_t sb[MAX_PHASE];
    *nchunks = plan_bounds(transpose ? h->ml : h->nl, h->xchunks, sb);
    for (int c = 0; c < 5; ++c) bounds[c] = sb[c];
    return PDLP_OK;
}

int pdlp_half_chunk(pdlp_handle h, int transpose, int chunk)
{
    if (!h || chunk < 0 || chunk >= MAX_CHUNKS) return PDLP_ERR_INVALID;
    if (transpose) return DISPATCH(h, half_chunk_t, h, true, h->yb[h->ix_cur], chunk);
    return DISPATCH(h, half_chunk_t, h, false, h->xbar, chunk);
}

int pdlp_tile_limits(pdlp_handle h, int32_t out[6])
{
    if (!h || !out) return PDLP_ERR_INVALID;
    out[4] = TNT;
    out[5] = 0;
    out[0] = h->rs_groups;
    out[1] = (int32_t)(h->part_blocks > INT32_MAX ? INT32_MAX : h->part_blocks);
    out[2] = h->p.dtype == PDLP_F64 ? TileCfg<double, double>::RPT_MAX : TileCfg<float, float>::RPT_MAX;
    out[3] = h->p.dtype == PDLP_F64 ? TileCfg<double, double>::CAP : TileCfg<float, float>::CAP;
    return PDLP_OK;
}

int pdlp_adaptive_retry(pdlp_handle h)
{
    if (!h) return PDLP_ERR_INVALID;
    if (h->delta || mid_split_product(h) || h->graph_ok || h->obj_mat.on) return PDLP_ERR_STATE;   // (float32 / float64 handles, between iterations, no Q)
    // the scalars: the rejected trial's weight leaves eta_total again, nothing is pending (the trial's epilogues have folded the
    // previous iterate's weight into the sums: the repeated half-steps must add nothing), k goes back; eta keeps the rule's eta'
    hipLaunchKernelGGL(k_retry_scalars, dim3(1), dim3(1), 0, h->stream, h->sc);
    HIP_TRY(hipGetLastError());
    // the iterate: the trial wrote x+, y+ into the "previous" buffers and made them current; the old (x, y) is intact in what is now
    // the previous pair
    const int t = h->ix_cur;
    h->ix_cur = h->ix_prev;
    h->ix_prev = t;
    h->carry.buffers_reassigned();
    h->carry.trial_undone();          // (kxb[0] belongs to the rejected x+, the running products of this period saw the trial)
    return PDLP_OK;
}

int pdlp_adaptive_reduce(pdlp_handle h)
{
    if (!h) return PDLP_ERR_INVALID;
    if (h->obj_mat.on) return PDLP_ERR_STATE;
    launch_adaptive_rule(h, 0);
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

int pdlp_adaptive_update(pdlp_handle h)
{
    if (!h) return PDLP_ERR_INVALID;
    if (h->obj_mat.on) return PDLP_ERR_STATE;
    WITH_T(h->p.dtype, hipLaunchKernelGGL(k_adaptive_update<T>, dim3(1), dim3(1), 0, h->stream, h->sc, h->red));
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

int pdlp_iterate(pdlp_handle h, int iters, int adaptive)
{
    if (!h || iters < 0) return PDLP_ERR_INVALID;
    adaptive = adaptive ? 1 : 0;
    if (adaptive && h->obj_mat.on) return PDLP_ERR_STATE;      // (sparse quadratic objective: fixed step only)
    h->carry.buffers_reassigned();
    char rname[64];
    if (g_roctx.level > 0) std::snprintf(rname, sizeof rname, "pdlp: %d %s iterations", iters, adaptive ? "adaptive" : "fixed-step");
    Range range(rname, h->stream);
    if (h->peer.on && h->peer.enabled) return iterate_peer(h, iters, adaptive);
    if (h->comm) return iterate_sharded(h, iters, adaptive);
    if (!whole_problem(h)) return PDLP_ERR_STATE;   // sharded without a communicator: the caller does the exchange
    return iterate_single(h, iters, adaptive);
}

// The adaptive iteration of a handle with a sparse quadratic objective: a mode of its own beside pdlp_iterate, whose refusal of
// adaptive != 0 on such a handle stands.  The forms without it are those without Q (pdlp_set_objective_matrix), and a handle on which
// the Halpern iteration has run since the last pdlp_set_iterate (PDLP_AVG holds its candidate, not an average).
int pdlp_objective_iterate(pdlp_handle h, int iters)
{
    if (!h || iters < 0) return PDLP_ERR_INVALID;
    if (!h->obj_mat.on || !plain_single(h) || h->graph_ok || h->carry.halpern || mid_split_product(h)) return PDLP_ERR_STATE;
    h->carry.buffers_reassigned();
    char rname[64];
    if (g_roctx.level > 0) std::snprintf(rname, sizeof rname, "pdlp: %d adaptive iterations (quadratic objective)", iters);
    Range range(rname, h->stream);
    return DISPATCH(h, objective_iterate_t, h, iters);
}

int pdlp_fixed_advance(pdlp_handle h, int iters)
{
    if (!h || iters < 0) return PDLP_ERR_INVALID;
    WITH_T(h->p.dtype, hipLaunchKernelGGL(k_fixed_advance<T>, dim3(1), dim3(1), 0, h->stream, h->sc, iters));
    HIP_TRY(hipGetLastError());
    return PDLP_OK;
}

int pdlp_flush_average(pdlp_handle h, int adaptive)
{
    if (!h) return PDLP_ERR_INVALID;
    if (h->carry.halpern) return PDLP_ERR_STATE;       // (the averaging calls would overwrite the Halpern candidate in PDLP_AVG)
    return DISPATCH(h, flush_t, h, adaptive ? 1 : 0);
}

int pdlp_compute_average(pdlp_handle h)
{
    if (!h) return PDLP_ERR_INVALID;
    if (h->carry.halpern) return PDLP_ERR_STATE;
    return DISPATCH(h, average_t, h);
}

int pdlp_kkt_local(pdlp_handle h, int which, int unscaled)
{
    if (!h || which < PDLP_CUR || which > PDLP_PREV) return PDLP_ERR_INVALID;
    Range range(which == PDLP_CUR ? "pdlp: KKT pass (current)" : which == PDLP_AVG ? "pdlp: KKT pass (average)" : "pdlp: KKT pass (previous)", h->stream);
    if (unscaled && (!h->p.d_col || !h->p.d_row)) return PDLP_ERR_STATE;
    if (h->delta) return delta_kkt_local(h, which, unscaled);
    return DISPATCH(h, kkt_local_t, h, which, unscaled);
}

int pdlp_report_local(pdlp_handle h, int which, int unscaled, void* rc_local, void* act_local)
{
    if (!h || which < PDLP_CUR || which > PDLP_PREV) return PDLP_ERR_INVALID;
    if (unscaled && (!h->p.d_col || !h->p.d_row)) return PDLP_ERR_STATE;
    if (mid_split_product(h) || h->range_sel >= 0) return PDLP_ERR_STATE;     // (nor between the pieces of a half-step)
    Range range("pdlp: solution report", h->stream);
    return DISPATCH(h, report_local_t, h, which, unscaled, rc_local, act_local);
}

int pdlp_read_red(pdlp_handle h, double out[PDLP_NRED])
{
    if (!h || !out) return PDLP_ERR_INVALID;
    HIP_TRY(hipMemcpyAsync(out, h->red, PDLP_NRED * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PDLP_OK;
}

int pdlp_kkt_finish(pdlp_handle h, double omega, double out[6])
{
    if (!h || !out) return PDLP_ERR_INVALID;
    double r[PDLP_NRED];
    int rc = pdlp_read_red(h, r);
    if (rc != PDLP_OK) return rc;
    DISPATCH(h, kkt_finish_t, r, omega, out);
    return PDLP_OK;
}

int pdlp_restart_distance_local(pdlp_handle h)
{
    if (!h) return PDLP_ERR_INVALID;
    return DISPATCH(h, distance_t, h);
}

int pdlp_mark_restart_point(pdlp_handle h)
{
    if (!h) return PDLP_ERR_INVALID;                                          // pdhg.py:63-64
    HIP_TRY(hipMemcpyAsync(h->x_last, h->xb[h->ix_cur] + h->p.col0 * h->es, h->nl * h->es, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->y_last, h->yb[h->ix_cur] + h->p.row0 * h->es, h->ml * h->es, hipMemcpyDeviceToDevice, h->stream));
    return PDLP_OK;
}

int pdlp_infeas_reset(pdlp_handle h)
{
    if (!h) return PDLP_ERR_INVALID;
    if (h->obj_diag || h->obj_mat.on) return PDLP_ERR_STATE;      // (no call of the detector with a quadratic objective)
    HIP_TRY(hipMemsetAsync(h->lam_prev, 0, h->nl * h->es, h->stream));          // pdhg.py:39-40
    return PDLP_OK;
}

int pdlp_infeas_begin(pdlp_handle h)
{
    if (!h) return PDLP_ERR_INVALID;
    if (has_extension(h)) return PDLP_ERR_STATE;       // (the detector's tests know one-sided rows and a linear objective only)
    return DISPATCH(h, infeas_begin_t, h);
}

int pdlp_infeas_local(pdlp_handle h, double tol)
{
    if (!h) return PDLP_ERR_INVALID;
    if (has_extension(h)) return PDLP_ERR_STATE;
    return DISPATCH(h, infeas_local_t, h, tol);
}

int pdlp_infeas_finish(pdlp_handle h, double tol, int32_t* status, double diag[8])
{
    if (!h || !status || !diag) return PDLP_ERR_INVALID;
    if (h->obj_diag || h->obj_mat.on) return PDLP_ERR_STATE;
    double r[PDLP_NRED];
    const int rc = pdlp_read_red(h, r);
    if (rc != PDLP_OK) return rc;
    *status = DISPATCH(h, infeas_decide_t, r, tol, diag);
    return PDLP_OK;
}

int pdlp_mv_steps(pdlp_handle h, int nvp, int steps, double eta, double omega, double theta, void* X, void* Y, void* work)
{
    if (!h || !X || !Y || !work || steps < 0 || (nvp != 8 && nvp != 16 && nvp != 32)) return PDLP_ERR_INVALID;
    if (!whole_problem(h) || h->mixed || has_extension(h)) return PDLP_ERR_STATE;   // (one-sided rows, linear objective)
    return DISPATCH(h, mv_steps_t, h, nvp, steps, eta, omega, theta, X, Y, work);
}

int pdlp_mv_gap(pdlp_handle h, int nvp, const void* X, const void* Y, void* work, double* gaps)
{
    if (!h || !X || !Y || !work || !gaps || (nvp != 8 && nvp != 16 && nvp != 32)) return PDLP_ERR_INVALID;
    if (!whole_problem(h) || h->mixed || has_extension(h)) return PDLP_ERR_STATE;   // (one-sided rows, linear objective)
    return DISPATCH(h, mv_gap_t, h, nvp, X, Y, work, gaps);
}

int pdlp_mv_product(pdlp_handle h, int nvp, const void* X, void* Y)
{
    if (!h || !X || !Y || (nvp != 8 && nvp != 16 && nvp != 32)) return PDLP_ERR_INVALID;
    if (!whole_problem(h) || h->mixed || has_extension(h)) return PDLP_ERR_STATE;   // (one-sided rows, linear objective)
    return DISPATCH(h, mv_product_t, h, nvp, X, Y);
}

int pdlp_spmv(pdlp_handle h, int transpose, const void* in_full, void* out_local)
{
    if (!h || !in_full || !out_local) return PDLP_ERR_INVALID;
    return DISPATCH(h, spmv_t, h, transpose, in_full, out_local);
}

int pdlp_power_iteration(pdlp_handle h, const void* b0, int iters, void* work_n, void* work_m, double* sigma)
{
    if (!h || !b0 || !work_n || !work_m || !sigma || iters < 0) return PDLP_ERR_INVALID;
    Range range("pdlp: power iteration", h->stream);
    if (!whole_problem(h)) return PDLP_ERR_STATE;
    return DISPATCH(h, power_iteration_t, h, b0, iters, work_n, work_m, sigma);
}

int pdlp_refresh_products(pdlp_handle h)
{
    if (!h) return PDLP_ERR_INVALID;
    Range range("pdlp: exact products (anchors / K x cache)", h->stream);
    if (h->delta) return delta_refresh(h);
    return DISPATCH(h, refresh_kx_t, h);
}

}  // extern "C"

#include "pdlp_batch_host.inc"
