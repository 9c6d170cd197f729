// pdlp_kernel_tiled.inc -- the panel-tiled kernel and the epilogue pass over partial row sums.
// Part of pdlp_hip.hip (included inside its anonymous namespace; not a translation unit of its own).
// ------------------------------------------------------------------------------------------------
// the panel-tiled kernel (format: torchpdlp_amd/tiled.py; float32 only).  A workgroup of 512 threads owns
// 512*rpt rows and walks the column panels in order; two workgroups share a CU (64 KB of LDS each) and all
// workgroups keep the same pace, so the 256 KB panel of the gathered vector stays in every XCD's L2.  Per tile:
//   pass 1  items are stored sorted by column (interleaved so that one gather instruction covers 64 consecutive
//           sorted items, i.e. few 128-byte lines): 16-byte streaming loads of (packed index, value) into
//           registers one group (8192 items) ahead, gathers, product stored to lds[slot] (slot = the item's rank
//           in row order: a transposition through LDS with plain stores, no atomics).  The waves raise their issue
//           priority for this pass (s_setprio): its memory instructions go out ahead of the other workgroup's pass-2
//           arithmetic;
//   pass 2  every thread owns rpt rows: their 4-bit segment lengths, a workgroup scan gives its first slot, and it
//           sums its segments into register accumulators (four items read unconditionally, item k weighted by
//           clamp(count - k, 0, 1)).  While one workgroup of the CU is in pass 2 the other one streams and gathers.
// Measured and not kept (round 2, 10M x 10M, ms per launch against 1.90-1.95 for this form in the same process):
//   LDS float atomics instead of pass 2 (ds_add_f32) 5.1; panels of 128K columns with half the rows per workgroup (fewer
//   (row, tile) pairs for pass 2, but half the items per gathered line) 2.5; the next tile's counts loaded during pass 2 2.2;
//   (that variant's loads sat behind `if (next tile exists)`: conditional loads make the compiler wait for everything; the
//   unconditional prefetch at the end of pass 1 that ships now gains 2 %);
//   two register buffers with the streaming loads issued behind the gathers (unconditional loads so that the compiler's wait
//   counts stay exact; chunks past a tile's end read cached lines) 2.3-2.5; all gathers of a group in flight at once (the
//   wave-uniform skip of chunks past the tile's end puts a branch between the chunks' gathers, and the compiler then waits for
//   chunk u's gathers before issuing chunk u+1's; without the skip -- chunks past the end gather one cached word -- 2.0-2.2; with the skip and an
//   explicit s_waitcnt vmcnt(0) at the top of the group, after which the chunks' gathers go out back to back, 2.01-2.12:
//   four gathers at a time per wave, one chunk after the other, is what the memory pipeline likes).
// float32 tile sets that qualify are read as 7-byte items (24-bit index words: the PACKED variant below, k_pack_items24).
// After the last panel the row sums go through LDS once more so that the epilogue runs with consecutive lanes
// on consecutive rows (coalesced vector traffic).
// ------------------------------------------------------------------------------------------------
#ifndef PDLP_PRIO_P1
#define PDLP_PRIO_P1 3                   /* s_setprio level of a wave in pass 1 (streaming loads, gathers, LDS stores) ... */
#define PDLP_PRIO_P2 0                   /* ... and in pass 2 / the epilogue */
#endif
#ifndef PDLP_GROUP_FAST
#define PDLP_GROUP_FAST 1                /* panel group = fast index of blockIdx in the split launches (XCD placement, see the kernel) */
#endif
#ifndef PDLP_EPI_GROUP
#define PDLP_EPI_GROUP 0                 /* rows whose epilogue operands are loaded together; 0: 8, or 4 for 8-byte operands */
#endif
#ifndef PDLP_TNT
#define PDLP_TNT 512                     /* threads per workgroup (lab builds: 1024 = one workgroup per CU with twice the rows) */
#endif
constexpr int TNT = PDLP_TNT;            // threads per workgroup
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
// per precision (T: vectors, products and row sums; TV: matrix values): most rows per thread (a multiple of 8: one 32-bit
// word holds 8 counts), most items per tile (LDS products: 64 KB and two workgroups per CU, or -- float32 values under
// float64 vectors, the "mixed" precision -- 128 KB and one workgroup per CU, so that ONE float32 tile set serves both the
// float32 kernel and this one), 4-item chunks per thread and register group, waves per SIMD the registers must allow
#ifndef PDLP_F32_RPT
#define PDLP_F32_RPT 40                  /* float32 tiles: most rows per thread (a multiple of 8) ... */
#define PDLP_F32_CAP 16384               /* ... most items per tile (LDS words of products per workgroup) ... */
#define PDLP_F32_TU 4                    /* ... 4-item chunks per thread and register group */
#endif
template <typename T, typename TV> struct TileCfg;
template <> struct TileCfg<float, float> { static constexpr int RPT_MAX = PDLP_F32_RPT, CAP = PDLP_F32_CAP, TU = PDLP_F32_TU, MINW = 4; typedef f32x4 V4; };
template <> struct TileCfg<double, double> { static constexpr int RPT_MAX = 24, CAP = 8192, TU = 2, MINW = 4; typedef f64x4 V4; };
template <> struct TileCfg<double, float> { static constexpr int RPT_MAX = PDLP_F32_RPT, CAP = PDLP_F32_CAP > 16384 ? 16384 : PDLP_F32_CAP, TU = 2, MINW = 2; typedef f32x4 V4; };
constexpr int TRPT_MAX_ANY = PDLP_F32_RPT > 40 ? PDLP_F32_RPT : 40;

__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float clamp01_t(float x) { return __builtin_amdgcn_fmed3f(x, 0.0f, 1.0f); }
__device__ __forceinline__ double clamp01_t(double x) { return __builtin_fmin(__builtin_fmax(x, 0.0), 1.0); }

// FUSED: the workgroup walks ALL panels of its row block and runs the epilogue itself.  Otherwise the panels of
// a row block are split over `groups` workgroups (blockIdx = group * nblk + row block; needed when there are too
// few rows for one workgroup per row block to fill the chip, e.g. one rank's shard of a sharded problem): each
// writes its partial row sums to rowsum[group] and k_rowsum_epilogue adds them in fixed order.
// PACKED (float32 only; format: pack_items24 in torchpdlp_amd/tiled.py, written by k_pack_items24 below): the index stream is 3 bytes
// per item instead of 4.  The four index words of a lane (one item of each of the chunk's four 64-item runs) are four little-endian
// 24-bit fields (slot << 10) | (local column - run base) in 12 bytes, and trb holds the four run bases of every 256-item chunk as
// four 16-bit numbers (8 bytes).  tidx then points to that stream (item offset i = byte 3 i) and only load_into / consume differ: one
// 12-byte streaming load per lane and chunk, the bases of a wave's TU chunks in ONE vector load requested ahead of the group's
// streaming loads (lane l gets word l & 1 of chunk (l >> 1) & 3; consume takes a base out with v_readlane), and gather j of a chunk
// reads (xin + base j) + 4 * (field & 1023): the base goes into the SCALAR part of the address, the vector part costs what it cost.
// (The bases as scalar loads, 16 scalar registers a group ahead, spilled: the 32-bit kernel already uses every scalar register, and
// spilled scalars land in vector registers, of which it has none to spare either.  One vector register holds all sixteen.)
// Same products into the same slots: bit for bit the sums of the 32-bit stream.
constexpr int P24_COL_BITS = 10, P24_SLOT_BITS = 14;
constexpr int P24_BASE_TAIL = TNT * 4 * TileCfg<float, float>::TU / 256;     // chunks a group may reach past the last tile's end: trb has that many spare (zero) entries
template <typename T, typename TV, class Epi, bool FUSED, bool PACKED = false>
__global__ __launch_bounds__(TNT, (TileCfg<T, TV>::MINW)) void k_tiled_fused(const uint32_t* __restrict__ tidx, const TV* __restrict__ tval,
                                                        const int32_t* __restrict__ tile_ptr, const int64_t* __restrict__ blk_base,
                                                        const uint32_t* __restrict__ tcnt, const uint32_t* __restrict__ trb,
                                                        int npanel, int lw, int rpt, int nrows, int nblk,
                                                        int vtotal, const int32_t* __restrict__ ptab, int slot0, int b0, int nbl,
                                                        const T* __restrict__ vin, T* __restrict__ rowsum,
                                                        int64_t rs_stride, const T* __restrict__ extra, Epi epi,
                                                        double* __restrict__ partials)
{
    typedef TileCfg<T, TV> Cfg;
    constexpr int TRPT_MAX = Cfg::RPT_MAX, TCW = TRPT_MAX / 8, TCAP = Cfg::CAP, TU = Cfg::TU;
    constexpr int TGRP = TNT * 4 * TU;       // items per register group
    typedef typename Cfg::V4 V4;
    __shared__ __attribute__((aligned(16))) T prod[TCAP + 8];
    __shared__ int wsum[TNT / 64];
    __shared__ double dred8[TNT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // (not FUSED: the launch covers the row blocks [b0, b0 + nbl) -- all of them, or the rows one piece of the NEXT exchange is
    //  made of, so that the piece can leave while the other rows are still being multiplied.
    //  XCD placement: workgroups are dealt round-robin over the 8 XCDs (blocks i and i + 8 share one; speed only, never
    //  correctness).  The GROUP is the fast index of blockIdx, so with 8 or 16 groups all workgroups of a panel group sit on ONE
    //  XCD and that XCD's L2 fetches only its groups' panels of the gathered vector -- row-block-fast numbering spread every group
    //  over all eight XCDs and each of them pulled the whole vector: 8 x 40 MB per product next to a rank's 1.1 GB of items.)
    const int ngrp = FUSED ? 1 : (int)(gridDim.x / (unsigned)nbl);
#if PDLP_GROUP_FAST
    const int b = FUSED ? blockIdx.x : b0 + (int)(blockIdx.x / (unsigned)ngrp);
    const int grp = FUSED ? 0 : (int)(blockIdx.x % (unsigned)ngrp);
#else       // (rounds 1-4, for A/B measurements: the row block is the fast index, every group is spread over all XCDs)
    const int b = FUSED ? blockIdx.x : b0 + (int)(blockIdx.x % (unsigned)nbl);
    const int grp = FUSED ? 0 : (int)(blockIdx.x / (unsigned)nbl);
#endif
    const int p_lo = (int)((int64_t)grp * vtotal / ngrp), p_hi = (int)((int64_t)(grp + 1) * vtotal / ngrp);
    // A launch walks `vtotal` panels in "virtual" order: panel = ptab[v] (ptab null: v itself).  That lets one launch cover
    // just the panels of the locally owned block of the gathered vector and others the panels whose entries arrive with the
    // first, second, ... chunk of the exchange (sharded problems: a launch runs while the rest of the vector is still in flight).
    // group g of n walks the virtual panels [g * vtotal / n, (g + 1) * vtotal / n): any n <= vtotal leaves no group empty
    auto pmap = [&](int v) { return ptab ? ptab[v] : v; };
    const uint32_t mask = (1u << lw) - 1u;
    if (FUSED) epi.load();
    T acc[TRPT_MAX];
#pragma unroll
    for (int r = 0; r < TRPT_MAX; ++r) acc[r] = (T)0;

    const uint32_t trash = (uint32_t)TCAP << lw;       // slot TCAP (past every real slot), column 0
    // the item stream is read once: non-temporal loads keep it from evicting the gathered panel out of the L2
    // One matrix copy may hold more than 2^31 items, but a row block never does: the block's position in the item arrays is a
    // 64-bit, wave-uniform number that goes into the base pointers once, and everything a thread indexes with is relative to it and
    // 32-bit (64-bit per-thread indices cost ten spilled registers and 7 % of the kernel: measured)
    static_assert(!PACKED || (sizeof(T) == 4 && sizeof(TV) == 4 && TCAP <= (1 << P24_SLOT_BITS)), "packed items: float32 tiles only");
    tidx += PACKED ? (blk_base[b] >> 2) * 3 : blk_base[b];       // (packed: 3 words per 4 items; the bases are multiples of 256 items)
    tval += blk_base[b];
    static_assert(!PACKED || TU == 4, "packed items: lane l holds bases of chunk (l >> 1) & 3");
    if (PACKED) trb += (blk_base[b] >> 8) * 2;                    // two words (four 16-bit run bases) per 256-item chunk
    // PACKED: pk[u].xyz are the lane's 12 bytes (w is not used); rbv: lanes 2u, 2u + 1 hold the four run bases of the wave's chunk u
    auto load_into = [&](u32x4 (&pk)[TU], V4 (&vv)[TU], uint32_t& rbv, int g0, int i1) {
        // the run bases first, so that they have landed when the first chunk's items have: an unconditional load (a chunk past the
        // tile's end reads the entry of whatever chunk lies there, or one of the P24_BASE_TAIL spare entries behind the last)
        // (PACKED addresses: uniform base + 32-bit byte offset per lane -- a row block of a packed tile set holds fewer than 2^30 items.
        //  The empty asm makes the group's position an opaque scalar, so the offsets are computed from it where they are used: left
        //  alone, the compiler turns every stream's address into a per-lane induction variable kept across the whole tile, as in the
        //  32-bit form -- 18 vector registers as 64-bit addresses, 9 as 32-bit offsets, and the kernel then spills 9 or 2)
        uint32_t gq = (uint32_t)g0 >> 2;
        if (PACKED) {
            asm volatile("" : "+s"(gq));
            const uint32_t ob = ((((gq >> 6) + ((lane >> 1) & (TU - 1)) * (TNT / 64) + wv) << 1) + (lane & 1)) << 2;
            rbv = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(trb) + ob);
        }
#pragma unroll
        for (int u = 0; u < TU; ++u) {
            const int i = g0 + (u * TNT + tid) * 4;
            if (i < i1) {
                if (PACKED) {
                    // three 4-byte loads of consecutive words: the compiler makes them ONE 12-byte load (global_load_dwordx3 ... nt; a
                    // 3-element vector type would be loaded as 16 bytes, one word past the lane's items and, at the very end, past the array)
                    const uint32_t i4 = gq + (uint32_t)(u * TNT + tid);               // = i / 4
                    const uint32_t* __restrict__ q = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(tidx) + i4 * 12u);
                    pk[u] = u32x4{__builtin_nontemporal_load(q), __builtin_nontemporal_load(q + 1), __builtin_nontemporal_load(q + 2), 0u};
                    vv[u] = __builtin_nontemporal_load(reinterpret_cast<const V4*>(reinterpret_cast<const char*>(tval) + i4 * 16u));
                } else {
                    pk[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(tidx + i));
                    vv[u] = __builtin_nontemporal_load(reinterpret_cast<const V4*>(tval + i));
                }
            } else {
                // (a wave's chunk is 256 aligned items and so are the tiles: it lies wholly inside a tile or wholly past its end, where
                //  consume skips it -- what is filled in here is never consumed; the 24-bit fields cannot name the trash slot, they get 0)
                pk[u] = PACKED ? u32x4{0u, 0u, 0u, 0u} : u32x4{trash, trash, trash, trash};
                vv[u] = V4{(TV)0, (TV)0, (TV)0, (TV)0};
            }
        }
    };
    // one register group: gathers, then the products go to their row-order slots in LDS.  Chunks of the group that
    // lie past the tile's end for this whole wave are skipped (wave-uniform).
    // A group is consumed in rounds of PDLP_ROUND items per lane (4 = one chunk): gathers of round r, then -- software pipeline --
    // the products of round r-1 go to LDS just before round r+1's gathers are issued, so the LDS stores run in the shadow of
    // the next gathers.  Each round sits in its own wave-uniform `if` (chunks past the tile's end are skipped); the compiler
    // waits for ALL outstanding loads before a conditional block with loads in it, i.e. a round's gathers land before the next
    // round's are issued.  That is the measured optimum, not an accident to repair (10M x 10M, ms per launch): 16 gathers per
    // lane in flight at once 2.0-2.1, rounds of 8: 2.0, rounds of 4 with the products in one burst at the end 1.90-1.95,
    // rounds of 4 pipelined 1.77-1.79.
#ifndef PDLP_ROUND
#define PDLP_ROUND 4
#endif
    auto consume = [&](u32x4 (&pk)[TU], V4 (&vv)[TU], uint32_t rbv, int g0, int i1, const T* __restrict__ xin) {
        constexpr int RPC = 4 / PDLP_ROUND, NR = TU * RPC;          // rounds per chunk, rounds per group
        T xg[TU * 4];
        bool on[TU];
#pragma unroll
        for (int u = 0; u < TU; ++u) on[u] = g0 + (u * TNT + __builtin_amdgcn_readfirstlane(wv) * 64) * 4 < i1;
        // PACKED: field k of the lane's 12 bytes in the low 24 bits (bits 24..31: the neighbouring field's, masked off by the users)
        auto pkw = [&](int u, int k) -> uint32_t {
            if (PACKED)
                return k == 0 ? pk[u].x : k == 1 ? __builtin_amdgcn_alignbit(pk[u].y, pk[u].x, 24)
                              : k == 2 ? __builtin_amdgcn_alignbit(pk[u].z, pk[u].y, 16) : pk[u].z >> 8;
            return k == 0 ? pk[u].x : k == 1 ? pk[u].y : k == 2 ? pk[u].z : pk[u].w;
        };
        auto rbw = [&](int u, int k) -> uint32_t { return ((uint32_t)__builtin_amdgcn_readlane((int)rbv, 2 * u + (k >> 1)) >> (16 * (k & 1))) & 0xffffu; };
        auto slot = [&](int u, int k) -> uint32_t { return PACKED ? (pkw(u, k) >> P24_COL_BITS) & ((1u << P24_SLOT_BITS) - 1u) : pkw(u, k) >> lw; };
        auto vvw = [&](int u, int k) -> TV { return k == 0 ? vv[u].x : k == 1 ? vv[u].y : k == 2 ? vv[u].z : vv[u].w; };
        auto products = [&](int r) {
            const int u = r / RPC, k0 = (r % RPC) * PDLP_ROUND;
            if (on[u]) {
#pragma unroll
                for (int k = k0; k < k0 + PDLP_ROUND; ++k) prod[slot(u, k)] = (T)vvw(u, k) * xg[4 * u + k];
            }
        };
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int u = r / RPC, k0 = (r % RPC) * PDLP_ROUND;
            if (r > 0) { products(r - 1); __builtin_amdgcn_sched_barrier(0); }
            if (on[u]) {
#pragma unroll
                for (int k = k0; k < k0 + PDLP_ROUND; ++k) {
                    if (PACKED)         // scalar base xin + run base, vector offset 4 * (field & 1023)
                        xg[4 * u + k] = *reinterpret_cast<const T*>(reinterpret_cast<const char*>(xin + rbw(u, k)) +
                                                                    ((pkw(u, k) << 2) & (((1u << P24_COL_BITS) - 1u) << 2)));
                    else
                        xg[4 * u + k] = *reinterpret_cast<const T*>(reinterpret_cast<const char*>(xin) + ((pkw(u, k) & mask) * (uint32_t)sizeof(T)));
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        products(NR - 1);
    };
    const size_t tile0 = (size_t)b * npanel;            // this row block's tiles in the count words ...
    const size_t tp0 = (size_t)b * (npanel + 1);        // ... and in tile_ptr (npanel + 1 offsets per row block)
    const bool has_panels = p_lo < vtotal;             // (the host never launches a group without panels)
    // The segment lengths of a tile: TCW words of eight 4-bit counts per thread.  Words 0..3 of all threads lie together as one
    // 16-byte entry per thread ([tile][thread][4]: one coalesced instruction, 8 lines per wave), the remaining TCW - 4 words
    // word-major behind all of those ([tile][word][thread]: 2 lines per wave and word).  Thread-major words ([tile][thread][TCW],
    // rounds 1-2) made every one of the TCW loads of a wave touch 10 lines for 256 bytes: 50 line visits per wave and tile.
    const size_t ntiles = (size_t)nblk * npanel;
    auto load_counts = [&](uint32_t (&cwd)[TCW], size_t tile) {
        const u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(tcnt) + tile * TNT + tid);
        cwd[0] = a.x;
        if (TCW > 1) cwd[1 < TCW ? 1 : 0] = a.y;
        if (TCW > 2) cwd[2 < TCW ? 2 : 0] = a.z;
        if (TCW > 3) cwd[3 < TCW ? 3 : 0] = a.w;
#pragma unroll
        for (int q = 4; q < TCW; ++q) cwd[q] = __builtin_nontemporal_load(tcnt + ntiles * TNT * 4 + (tile * (TCW > 4 ? TCW - 4 : 1) + (q - 4)) * TNT + tid);
    };
    u32x4 pk[TU];
    uint32_t rbv = 0;
    V4 vv[TU];
    int i0 = has_panels ? tile_ptr[tp0 + pmap(p_lo)] : 0;
    int i1 = has_panels ? tile_ptr[tp0 + pmap(p_lo) + 1] : 0;
    load_into(pk, vv, rbv, i0, i1);

    for (int i = tid; i < TCAP + 8; i += TNT) prod[i] = (T)0;      // pass 2 reads past short rows with weight 0: never uninitialised words
    __syncthreads();
    // (the next tile's segment lengths loaded during pass 2 of this one, word by word as the registers come free, measured
    // SLOWER: 1.87 -> 2.19 ms; they are loaded at the top of their tile)
    uint32_t cwn[TCW];
    {
        load_counts(cwn, tile0 + (has_panels ? pmap(p_lo) : 0));
    }
    for (int v = p_lo; v < p_hi; ++v) {
        const int p = pmap(v);
        const T* __restrict__ xin = vin + ((size_t)p << lw);
        int i0n = i1, i1n = i1;                                                  // the next tile (empty after the last)
        if (v + 1 < p_hi) {
            const int pn = pmap(v + 1);
            i0n = tile_ptr[tp0 + pn];
            i1n = tile_ptr[tp0 + pn + 1];
        }
        // segment lengths (4 bits each) of this thread's rows: row i of lane l of wave w is row w*64*rpt + i*64 + l
        // of the row block, so the 64 lanes of a wave sit on 64 consecutive rows for every i
        uint32_t cw[TCW];
        uint32_t total = 0;
#pragma unroll
        for (int q = 0; q < TCW; ++q) cw[q] = cwn[q];    // requested at the end of the previous tile's pass 1
#pragma unroll
        for (int q = 0; q < TCW; ++q) {
            const uint32_t n2 = (cw[q] & 0x0f0f0f0fu) + ((cw[q] >> 4) & 0x0f0f0f0fu);
            total += (n2 * 0x01010101u) >> 24;
        }
        total = wave_incl_scan_u32(total);
        if (lane == 63) wsum[wv] = (int)total;           // items of this wave's rows in this tile
        // pass 1, one register group at a time; the next group (of this tile or of the next) is loaded as soon as
        // the current one is consumed
        // the streaming / gathering phase issues ahead of the other workgroup's reduction phase (its VALU work would
        // otherwise delay the memory instructions everything waits for: 2.07 -> 1.87 ms per launch at 10M x 10M)
        __builtin_amdgcn_s_setprio(PDLP_PRIO_P1);
        for (int g0 = i0; g0 < i1; g0 += TGRP) {
            consume(pk, vv, rbv, g0, i1, xin);
            if (g0 + TGRP < i1) load_into(pk, vv, rbv, g0 + TGRP, i1);
            else load_into(pk, vv, rbv, i0n, i1n);
        }
        if (i0 >= i1) load_into(pk, vv, rbv, i0n, i1n);       // (an empty tile consumed nothing)
        {   // the next tile's segment lengths: unconditional loads (after the last tile: this tile's again), behind the streaming
            // loads of the next group; they have pass 2 and two barriers to land
            load_counts(cwn, tile0 + (v + 1 < p_hi ? pmap(v + 1) : p));
        }
        __builtin_amdgcn_s_setprio(PDLP_PRIO_P2);
        __syncthreads();
        int sb = 0;
#pragma unroll
        for (int w = 0; w < TNT / 64; ++w) sb += (w < wv) ? wsum[w] : 0;
        uint32_t sbase = (uint32_t)__builtin_amdgcn_readfirstlane(sb);      // first slot of this wave's rows
        // pass 2: segment sums.  The slots are in row order, so for a given i the 64 rows of the wave own one
        // contiguous run of slots: a row's first slot is the wave's running base plus the exclusive scan of the
        // lanes' counts.  Four row indices are scanned at once (8-bit fields of one word; the format guarantees
        // that 64 consecutive rows hold fewer than 256 items of a tile).  Consecutive lanes then read (nearly)
        // consecutive LDS words -- the earlier thread-owns-consecutive-rows mapping put lanes ~26 words apart
        // and paid 4-way bank conflicts on every read.  The first four items of every row are read
        // unconditionally and selected by the row's count (no load-to-use chains, no exec masking; reading past
        // a short row touches the next rows' items or the 8-word tail of the buffer); longer segments (0.06 % of
        // the (row, tile) pairs at 0.65 items per pair) finish in a loop.
#pragma unroll
        for (int q = 0; q < TCW; ++q) {
            if (8 * q < rpt) {
                uint32_t cE = cw[q] & 0x0f0f0f0fu, cO = (cw[q] >> 4) & 0x0f0f0f0fu;           // rows 8q+{0,2,4,6} | 8q+{1,3,5,7}
                asm("" : "+v"(cE), "+v"(cO));            // (byte fields from here on: conversions straight from the packed word)
                uint32_t sE = cE, sO = cO;
                wave_incl_scan2_u32(sE, sO);
                const uint32_t tE = (uint32_t)__builtin_amdgcn_readlane((int)sE, 63), tO = (uint32_t)__builtin_amdgcn_readlane((int)sO, 63);
                const uint32_t eE = sE - cE, eO = sO - cO;                                    // exclusive, field by field
                constexpr int RG = sizeof(T) == 8 ? 2 : 4;      // rows advanced together (register budget)
#pragma unroll
                for (int g = 0; g < 8 / RG; ++g) {
                    if (8 * q + RG * g < rpt) {         // counts of rows >= rpt are zero
                        int cc[RG], oo[RG];
#pragma unroll
                        for (int z = 0; z < RG; ++z) {
                            const int j = (RG * g + z) >> 1;                                  // field
                            const bool odd = (RG * g + z) & 1;
                            cc[z] = (int)(((odd ? cO : cE) >> (8 * j)) & 0xffu);
                            oo[z] = (int)(sbase + (((odd ? eO : eE) >> (8 * j)) & 0xffu));
                            sbase += ((odd ? tO : tE) >> (8 * j)) & 0xffu;
                        }
                        T v[RG * 4];
#pragma unroll
                        for (int z = 0; z < RG; ++z)
#pragma unroll
                            for (int k = 0; k < 4; ++k) v[4 * z + k] = prod[oo[z] + k];
#pragma unroll
                        for (int z = 0; z < RG; ++z) {
                            // item k counts with weight clamp(c - k, 0, 1): one clamped add and one fused multiply-add per
                            // item (x * 1 + a rounds once, like a + x; what is read past a short row gets weight 0 -- LDS
                            // holds products or the zeros it was cleared to, and 0 * finite = 0)
                            T cf = (T)(((((RG * g + z) & 1) ? cO : cE) >> (8 * ((RG * g + z) >> 1))) & 0xffu);    // v_cvt_f32_ubyteN
                            asm("" : "+v"(cf));          // (keeps the subtractions on the float side: v_add_f32 ... clamp)
                            T a = acc[8 * q + RG * g + z];
                            a = fma_t(v[4 * z], clamp01_t(cf), a);
                            a = fma_t(v[4 * z + 1], clamp01_t(cf - (T)1), a);
                            a = fma_t(v[4 * z + 2], clamp01_t(cf - (T)2), a);
                            a = fma_t(v[4 * z + 3], clamp01_t(cf - (T)3), a);
                            if (cf > (T)4) {
                                int k = 4;
#pragma nounroll
                                do a += prod[oo[z] + k]; while (++k < cc[z]);      // (rare: kept small, 40 copies of it sit in the hot loop's code)
                            }
                            acc[8 * q + RG * g + z] = a;
                        }
                    }
                }
            }
        }
        __syncthreads();
        i0 = i0n;
        i1 = i1n;
    }
    // The row sums sit in registers, lane l of wave w holding rows w*64*rpt + i*64 + l: for every i the lanes are
    // on consecutive rows, so the epilogue (or the store of the partial sums) is coalesced straight from registers.
    const int rb = TNT * rpt;
    const int row0 = b * rb + wv * 64 * rpt + lane;
    if (!FUSED) {
        T* __restrict__ rs = rowsum + (size_t)(slot0 + grp) * rs_stride;
#pragma unroll
        for (int r = 0; r < TRPT_MAX; ++r)
            if (r < rpt && row0 + 64 * r < nrows) rs[row0 + 64 * r] = acc[r];
        return;
    }
    double accd[NACC] = {0.0, 0.0, 0.0, 0.0};
    // The epilogue's operand loads are issued for EG rows at a time before any of them is used: one row after the other (load,
    // wait, compute, store, 40 times) left every workgroup in a chain of 40 memory round trips at the very end of the kernel,
    // when nothing else is in flight -- each extra operand stream cost 0.04 ms there (measured).  Rows past the end are loaded
    // from the last row (valid memory) and not stored.
    constexpr int EG = PDLP_EPI_GROUP > 0 ? PDLP_EPI_GROUP : (sizeof(typename Epi::Pre) <= 24 ? 8 : 4);     // (8 rows of 48-byte operand sets spill)
    const int lastrow = nrows - 1;
    // extra: the remainder's row sums (items the tile format could not hold; null when there are none)
    if (extra) {
#pragma unroll
        for (int r0 = 0; r0 < TRPT_MAX; r0 += EG) {
            if (r0 < rpt) {
                T ex[EG];
#pragma unroll
                for (int g = 0; g < EG; ++g) {
                    const int row = row0 + 64 * (r0 + g);
                    ex[g] = extra[row < lastrow ? row : lastrow];
                }
#pragma unroll
                for (int g = 0; g < EG; ++g)
                    if (r0 + g < TRPT_MAX) acc[r0 + g < TRPT_MAX ? r0 + g : 0] += ex[g];
            }
        }
    }
#pragma unroll
    for (int r0 = 0; r0 < TRPT_MAX; r0 += EG) {
        if (r0 < rpt) {
            typename Epi::Pre pre[EG];
#pragma unroll
            for (int g = 0; g < EG; ++g) {
                const int row = row0 + 64 * (r0 + g);
                pre[g] = epi.pre(row < lastrow ? row : lastrow);
            }
#pragma unroll
            for (int g = 0; g < EG; ++g) {
                const int row = row0 + 64 * (r0 + g);
                if (r0 + g < TRPT_MAX && r0 + g < rpt && row < nrows) epi(row, acc[r0 + g < TRPT_MAX ? r0 + g : 0], pre[g], accd);
            }
        }
    }
    if (Epi::NA > 0) {
#pragma unroll
        for (int r = 0; r < Epi::NA; ++r) {
            double v = accd[r];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += shfl_xor_t(v, off);
            __syncthreads();
            if (lane == 0) dred8[wv] = v;
            __syncthreads();
            if (tid == 0) {
                double t = 0.0;
                for (int w = 0; w < TNT / 64; ++w) t += dred8[w];
                partials[(size_t)b * NACC + r] = t;
            }
        }
    }
}

// epilogue of the split tiled kernel: row sum = sum over panel groups (fixed order), then the fused vector update
template <typename T, class Epi>
__global__ __launch_bounds__(BLOCK) void k_rowsum_epilogue(const T* __restrict__ rowsum, int groups, int64_t rs_stride,
                                                           int nrows, const T* __restrict__ extra, Epi epi,
                                                           double* __restrict__ partials, int row_lo = 0)
{
    // rows [row_lo, nrows): all rows, or the rows of one piece of the next exchange (its own launch, its own partial-sum slots)
    __shared__ double dred[4];
    epi.load();
    double acc[NACC] = {0.0, 0.0, 0.0, 0.0};
    for (int row = row_lo + blockIdx.x * BLOCK + threadIdx.x; row < nrows; row += gridDim.x * BLOCK) {
        // the epilogue's operands first, then the partial sums four groups at a time: unconditional loads on clamped group
        // indices (a group past the last re-reads the last one and is not added), so a batch is one memory round trip -- the
        // plain loop was one round trip per group, plus one for the operands
        const typename Epi::Pre pre = epi.pre(row);
        T s = (T)0;                                                              // groups == 0: no product part (vector pass only)
        const int glast = groups - 1;
        for (int g0 = 0; g0 < groups; g0 += 4) {
            T part[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int g = g0 + k < glast ? g0 + k : glast;
                part[k] = __builtin_nontemporal_load(rowsum + (size_t)g * rs_stride + row);
            }
            s = g0 == 0 ? part[0] : s + part[0];                                  // (fixed order, exactly the plain loop's)
#pragma unroll
            for (int k = 1; k < 4; ++k) s = g0 + k < groups ? s + part[k] : s;
        }
        if (extra) s += extra[row];
        epi(row, s, pre, acc);
    }
    if (Epi::NA > 0) {
#pragma unroll
        for (int r = 0; r < Epi::NA; ++r) {
            const double v = block_sum(acc[r], dred);
            if (threadIdx.x == 0) partials[(size_t)blockIdx.x * NACC + r] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// the packed index stream of a float32 tile set, made once from the 32-bit one (k_tiled_fused<..., PACKED>; the CPU model is
// pack_items24 in torchpdlp_amd/tiled.py).  One wave per 256-item chunk: lane l holds positions 4l..4l+3, i.e. sorted items 64j + l
// of the chunk's runs j = 0..3.  Padding items sit at the end of a tile's sorted order and all carry the same word (slot = the
// tile's number of real items, column 0), so inside a chunk they are the items equal to the chunk's LAST sorted item when that one
// has column 0 (if that item is a real one, every item of the chunk has column 0 and nothing depends on the distinction).  Run base =
// smallest local column of the run's real items (0 for a run of padding); field = (slot << 10) | (column - base), column part 0 for
// padding; the four bases of a chunk are stored as 16-bit numbers in two words (lw <= 16).  *flag is raised when a field does not
// fit: a run spanning more than 1023 columns or a slot above 16383.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_pack_items24(const uint32_t* __restrict__ idx, int64_t nchunks, int lw, uint32_t* __restrict__ idx24,
                                                        uint32_t* __restrict__ run_base, int32_t* __restrict__ flag)
{
    const int lane = threadIdx.x & 63;
    const uint32_t mask = (1u << lw) - 1u;
    const int64_t stride = (int64_t)gridDim.x * (BLOCK / 64);
    for (int64_t c = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); c < nchunks; c += stride) {
        const u32x4 w4 = *(reinterpret_cast<const u32x4*>(idx) + c * 64 + lane);
        const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
        const uint32_t last = (uint32_t)__builtin_amdgcn_readlane((int)w4.w, 63);
        const bool has_pad = (last & mask) == 0u;
        uint32_t f[4], rb[4];
        bool bad = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool pad = has_pad && w[j] == last;
            const uint32_t col = w[j] & mask, sl = w[j] >> lw;
            uint32_t m = pad ? 0xffffffffu : col;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)m, off, 64);
                m = o < m ? o : m;
            }
            rb[j] = m == 0xffffffffu ? 0u : m;
            const uint32_t d = pad ? 0u : col - rb[j];
            bad = bad || d >= (1u << P24_COL_BITS) || sl >= (1u << P24_SLOT_BITS);
            f[j] = ((sl & ((1u << P24_SLOT_BITS) - 1u)) << P24_COL_BITS) | (d & ((1u << P24_COL_BITS) - 1u));
        }
        uint32_t* __restrict__ o = idx24 + (c * 64 + lane) * 3;
        o[0] = f[0] | (f[1] << 24);
        o[1] = (f[1] >> 8) | (f[2] << 16);
        o[2] = (f[2] >> 16) | (f[3] << 8);
        if (lane < 2) run_base[c * 2 + lane] = lane ? rb[2] | (rb[3] << 16) : rb[0] | (rb[1] << 16);
        if (bad) *flag = 1;
    }
}

// ------------------------------------------------------------------------------------------------
// the remainder of a tiled matrix (torchpdlp_amd/tiled.py): the items its tiles could not hold, as segments of <= 512 items of
// the rows that have any.  Eight lanes per segment; then eight lanes per row add the row's segment sums and write
// the row's entry of the dense `extra` vector, which is zero everywhere else and stays so (the same rows are rewritten by
// every product).  Fixed summation order => deterministic.
// ------------------------------------------------------------------------------------------------
template <typename T, typename TV>
__global__ __launch_bounds__(BLOCK) void k_rem_segments(int ns, const int32_t* __restrict__ sptr, const int32_t* __restrict__ col,
                                                        const TV* __restrict__ val, const T* __restrict__ vin, T* __restrict__ seg_sum)
{
    // eight lanes per segment (<= 512 items; most segments of a real remainder hold a handful), lanes strided over the items, eight
    // items per lane and round trip (all item loads, then all gathers: unconditional on clamped indices), shuffle tree over the
    // eight lanes.  (One wave per segment, the first form, spent 146 us on the 600k short segments a dense column leaves.)
    const int lt = threadIdx.x & 7;
    const int64_t stride = ((int64_t)gridDim.x * BLOCK) >> 3;
    const int64_t ns_pad = ((int64_t)ns + stride - 1) / stride * stride;               // whole groups stay together for the shuffles
    for (int64_t g = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 3; g < ns_pad; g += stride) {
        T s = (T)0;
        if (g < ns) {
            const int a = sptr[g], nn = sptr[g + 1] - a;
            const int last = nn - 1;
            for (int i0 = lt; i0 < nn; i0 += 64) {
                T lv[8], lg[8];
                int lc[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = i0 + 8 * u, ic = i < last ? i : last;
                    lv[u] = (T)val[a + ic];
                    lc[u] = col[a + ic];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) lg[u] = vin[lc[u]];
#pragma unroll
                for (int u = 0; u < 8; ++u) s = i0 + 8 * u < nn ? s + lv[u] * lg[u] : s;
            }
        }
        for (int off = 4; off > 0; off >>= 1) s += shfl_xor_t(s, off);
        if (g < ns && lt == 0) seg_sum[g] = s;
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_rem_rows(int nr, const int32_t* __restrict__ rows, const int32_t* __restrict__ rptr,
                                                    const T* __restrict__ seg_sum, T* __restrict__ extra)
{
    // eight lanes per row, strided over the row's segment sums (a dense row of 2M items has 4k of them), shuffle tree
    const int lt = threadIdx.x & 7;
    const int64_t stride = ((int64_t)gridDim.x * BLOCK) >> 3;
    const int64_t nr_pad = ((int64_t)nr + stride - 1) / stride * stride;             // whole groups stay together for the shuffles
    for (int64_t i = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 3; i < nr_pad; i += stride) {
        T s = (T)0;
        if (i < nr) {
            // eight loads in flight per lane (unconditional, clamped to the row's last segment; same order of additions as the
            // plain loop): a dense row of 2M items has 4k segment sums, i.e. 512 per lane -- one load per round trip made this
            // kernel 0.2 ms of a 2 ms product
            const int g0 = rptr[i], g1 = rptr[i + 1];
            for (int g = g0 + lt; g < g1; g += 64) {
                T part[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int gk = g + 8 * k;
                    part[k] = seg_sum[gk < g1 ? gk : g1 - 1];
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) s = g + 8 * k < g1 ? s + part[k] : s;
            }
        }
        for (int off = 4; off > 0; off >>= 1) s += shfl_xor_t(s, off);
        if (i < nr && lt == 0) extra[rows[i]] = s;
    }
}

// red[off + r] = sum over blocks of partials[b][r]   (one workgroup; fixed order => deterministic)
__global__ __launch_bounds__(BLOCK) void k_finalize(const double* __restrict__ partials, int nblocks, int na,
                                                    double* __restrict__ red, int off)
{
    __shared__ double dred[4];
    for (int r = 0; r < na; ++r) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += BLOCK) s += partials[(size_t)b * NACC + r];
        s = block_sum(s, dred);
        if (threadIdx.x == 0) red[off + r] = s;
        __syncthreads();
    }
}
