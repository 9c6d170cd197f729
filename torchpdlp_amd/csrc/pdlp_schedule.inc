// pdlp_schedule.inc -- how the work of a product is cut up: the row-block and long-row schedules of the CSR kernel, built on the
// host and uploaded at pdlp_create (K, K') or by pdlp_set_objective_matrix (Q, into the caller's memory); the pieces of a chunked exchange (plan_bounds); and the planner of a sharded problem's split
// products (configure_split: which panels belong to which phase of the exchange, how many panel groups each phase gets, in which
// pieces the result leaves), with the helpers that turn an output piece into rows and grids.
// Part of pdlp_hip.hip (included at file scope; not a translation unit of its own).  Needs: pdlp_handle.inc.
// ------------------------------------------------------------------------------------------------
namespace {

void build_long_rows_host(const std::vector<int64_t>& rp, int64_t rows, std::vector<int64_t>& lch, std::vector<int32_t>& lrow,
                          std::vector<int32_t>& lptr)
{
    lch.clear(); lrow.clear(); lptr.clear();
    lptr.push_back(0);
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t a = rp[r], e = rp[r + 1];
        if (e - a <= NNZ_CAP) continue;
        for (int64_t c = a; c < e; c += NNZ_CAP) {
            lch.push_back(c);
            lch.push_back(c + NNZ_CAP < e ? c + NNZ_CAP : e);
        }
        lrow.push_back((int32_t)r);
        lptr.push_back((int32_t)(lch.size() / 2));
    }
}

// out = (first row, first non-zero) of every block, then (rows, nnz) as the end marker: 2 * (blocks + 1) entries
void build_schedule_host(const std::vector<int64_t>& rp, int64_t rows, std::vector<int64_t>& out)
{
    out.clear();
    int64_t r = 0;
    out.push_back(0);
    out.push_back(0);
    while (r < rows) {
        int64_t e = r;
        int64_t nnz = 0;
        while (e < rows && e - r < ROWS_CAP) {
            const int64_t len = (int64_t)rp[e + 1] - rp[e];
            if (nnz + len > NNZ_CAP) break;
            nnz += len;
            ++e;
        }
        if (e == r) e = r + 1;   // a single row longer than NNZ_CAP: its own (skipped) block, done in chunks
        out.push_back(e);
        out.push_back(rp[e]);
        r = e;
    }
}

// One matrix's tables into the device arrays `sc` points at: the row pointers' low words, the row-block schedule and the long-row
// tables, with the grids that follow from them.  Every copy is on the caller's stream and waited for (the host vectors go away;
// later work on that stream is ordered behind it).
int upload_schedule(pdlp_handle h, Schedule& sc, const std::vector<int64_t>& rp, int64_t rows)
{
    auto upload = [&](void* dst, const void* src, size_t bytes) {
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream) == hipSuccess && hipStreamSynchronize(h->stream) == hipSuccess;
    };
    const int fail = PDLP_ERR_HIP_BASE - 1;
    const std::vector<uint32_t> lo(rp.begin(), rp.end());    // (truncating: the low 32 bits)
    if (!upload(sc.rplo, lo.data(), lo.size() * 4)) return fail;
    std::vector<int64_t> sched;
    build_schedule_host(rp, rows, sched);
    sc.nblk = rows > 0 ? (int)sched.size() / 2 - 1 : 0;
    if (!upload(sc.blk, sched.data(), sched.size() * 8)) return fail;
    // rows longer than NNZ_CAP
    std::vector<int64_t> lch;
    std::vector<int32_t> lrow, lptr;
    build_long_rows_host(rp, rows, lch, lrow, lptr);
    sc.nchunks = (int)(lch.size() / 2); sc.nlong = (int)lrow.size();
    sc.lgrid = sc.nlong > 0 ? (int)((sc.nlong + BLOCK - 1) / BLOCK < LONG_GRID ? (sc.nlong + BLOCK - 1) / BLOCK : LONG_GRID) : 0;
    const int64_t work = (int64_t)sc.nblk + sc.nchunks;
    sc.grid = (int)(work < MAX_GRID ? work : MAX_GRID);
    if (sc.nlong > 0) {
        if (!upload(sc.lch, lch.data(), lch.size() * 8) || !upload(sc.lrow, lrow.data(), lrow.size() * 4) ||
            !upload(sc.lptr, lptr.data(), lptr.size() * 4))
            return fail;
    }
    return PDLP_OK;
}

// Everything pdlp_create uploads into the handle's workspace (bind_layout has set the pointers): the tables of K and K'.
int upload_schedules(pdlp_handle h, const std::vector<int64_t>& rpK, const std::vector<int64_t>& rpKT)
{
    const int rc = upload_schedule(h, h->sK, rpK, h->ml);
    return rc == PDLP_OK ? upload_schedule(h, h->sKT, rpKT, h->nl) : rc;
}

// The third schedule, of the objective's matrix Q (pdlp_set_objective_matrix): the same tables, carved out of the caller's `work` in
// the order low words, block pairs, long-row tables.  objective_matrix_layout is the one place that knows the sizes (the size query
// and the setter both call it).  At the end: the partial sums of the step product's curvature (pdlp_objective_iterate) -- partA and
// partB hold the half-steps' sums when the step-size rule reads all three -- for as many workgroups as a product with Q can have
// (grid_of(sQ, n): at most MAX_GRID row-block workgroups and LONG_GRID of the long rows, and never more than there is work).
struct ObjMatrixLayout { int64_t rplo, blk, lch, lrow, lptr, longpart, part, bytes; };
inline int64_t objective_part_blocks(int64_t n, int64_t nnz)
{
    const int64_t work = max_blocks(n, nnz) + max_chunks(nnz), lg = (max_long(nnz) + BLOCK - 1) / BLOCK;
    return (work < MAX_GRID ? work : MAX_GRID) + (lg < LONG_GRID ? lg : LONG_GRID);
}
inline ObjMatrixLayout objective_matrix_layout(int64_t n, int64_t nnz, int64_t es)
{
    ObjMatrixLayout L{};
    Carve c;
    L.rplo = c.take((n + 1) * 4);
    L.blk = c.take((max_blocks(n, nnz) + 1) * 16);
    L.lch = c.take(max_chunks(nnz) * 2 * 8);
    L.lrow = c.take(max_long(nnz) * 4);
    L.lptr = c.take((max_long(nnz) + 1) * 4);
    L.longpart = c.take(max_chunks(nnz) * es);
    L.part = c.take(objective_part_blocks(n, nnz) * NACC * 8);
    L.bytes = c.off;
    return L;
}

int upload_objective_schedule(pdlp_handle h, const std::vector<int64_t>& rp, char* work)
{
    const int64_t n = h->p.n;
    const ObjMatrixLayout L = objective_matrix_layout(n, rp[(size_t)n], (int64_t)h->es);
    Schedule sc;
    sc.rplo = (uint32_t*)(work + L.rplo); sc.blk = (int64_t*)(work + L.blk);
    sc.lch = (int64_t*)(work + L.lch); sc.lrow = (int32_t*)(work + L.lrow); sc.lptr = (int32_t*)(work + L.lptr);
    sc.longpart = (void*)(work + L.longpart);
    const int rc = upload_schedule(h, sc, rp, n);
    if (rc == PDLP_OK) { h->sQ = sc; h->obj_mat.part = (double*)(work + L.part); }
    return rc;
}

// Output pieces of a split product (Schedule::nrange > 1): rows of piece r = row blocks [rb_lo[r], rb_lo[r+1]).  The k_rowsum_epilogue
// launches of the pieces write their partial sums one after the other: piece r's first slot, and the total.
inline int range_rows_lo(const Schedule& s, int r) { return s.rb_lo[r] * TNT * s.t.rpt; }
inline int range_rows_hi(const Schedule& s, int r, int rows) { const int64_t e = (int64_t)s.rb_lo[r + 1] * TNT * s.t.rpt; return (int)(e < rows ? e : rows); }
inline int range_epi_grid(const Schedule& s, int r, int rows)
{
    return rows_grid(range_rows_hi(s, r, rows) - range_rows_lo(s, r));
}
inline int split_epi_grid(const Schedule& s, int rows)
{
    if (s.nrange <= 1) return grid_for(rows);
    int g = 0;
    for (int r = 0; r < s.nrange; ++r) g += range_epi_grid(s, r, rows);
    return g;
}

// The pieces of a chunked exchange: piece c moves elements [sb[c], sb[c+1]) of every rank's block of `B` elements (multiples of
// 64 elements: 256-byte pieces).  A function of B and the requested count alone -- every rank computes the same plan, whether
// or not its own product is split (the collectives must match on all ranks; what a rank multiplies early is its own business).
int plan_bounds(int64_t B, int xchunks, int64_t* sb /*[MAX_PHASE]*/)
{
    int C = xchunks < 1 ? 1 : (xchunks > MAX_CHUNKS ? MAX_CHUNKS : xchunks);
    if (B < (int64_t)64 * C) C = 1;
    for (int c = 0; c <= C; ++c) sb[c] = c == C ? B : (c * B / C) / 64 * 64;
    for (int c = C + 1; c < MAX_PHASE; ++c) sb[c] = B;
    return C;
}

// panel groups of the split product of one matrix (see Schedule): which panels belong to which phase of the exchange, and how
// many workgroup groups (= partial row sum slots) every phase gets
int configure_split(pdlp_handle h, bool transpose)
{
    Schedule& s = transpose ? h->sKT : h->sK;
    s.loc_pa = s.loc_pb = s.slotsA = s.slotsB = 0;
    s.pending = false;
    s.nphase = 0; s.chunks_done = 0;
    s.nrange = 0;
    if (!s.tiled) return PDLP_OK;
    const int64_t lo = transpose ? h->p.row0 : h->p.col0, hi = transpose ? h->p.row1 : h->p.col1;
    const int64_t total = transpose ? h->p.m : h->p.n;
    if (lo == 0 && hi == total) return PDLP_OK;                       // not sharded: nothing to wait for
    const int64_t W = (int64_t)1 << s.t.lw, B = hi - lo;
    const int npanel = s.t.npanel;
    const int pa = (int)((lo + W - 1) / W), pb = hi == total ? npanel : (int)(hi / W);
    const int nloc = pb - pa, nrem = npanel - nloc;
    if (nloc <= 0 || nrem <= 0 || h->rs_groups < 2 || !s.ptab || npanel > s.ptab_cap || B <= 0 || lo % B != 0) return PDLP_OK;
    const int C = plan_bounds(B, h->xchunks, s.sb);
    // The RESULT of this product (this rank's block of y for K, of xbar for K') is the input of the other product and travels in
    // the pieces of THAT exchange: elements [so[r], so[r+1]) of the block = piece r.  With more than one piece the last phase and
    // the epilogue run piece by piece (launch_mat): the row blocks that hold piece r's rows, then piece r + 1's.
    const int64_t rows_out = transpose ? h->nl : h->ml;
    const int64_t rbk = (int64_t)TNT * s.t.rpt;
    int64_t so[MAX_PHASE];
    const int R = h->producer_pieces ? plan_bounds(rows_out, h->xchunks, so) : 1;
    int nb_max = s.t.nblk;
    if (R > 1) {
        nb_max = 0;
        for (int r = 0; r <= R; ++r) {
            const int64_t b = r == R ? s.t.nblk : (so[r] + rbk - 1) / rbk;
            s.rb_lo[r] = (int)(b < s.t.nblk ? b : s.t.nblk);
        }
        for (int r = 0; r < R; ++r) nb_max = (s.rb_lo[r + 1] - s.rb_lo[r]) > nb_max ? (s.rb_lo[r + 1] - s.rb_lo[r]) : nb_max;
    }
    // a panel is complete once the last of its foreign entries has arrived
    std::vector<int> phase((size_t)npanel);
    int cnt[MAX_PHASE] = {0};
    for (int p = 0; p < npanel; ++p) {
        int ph = 0;
        if (p < pa || p >= pb) {
            const int64_t c0 = (int64_t)p * W, c1 = (c0 + W < total) ? c0 + W : total;
            ph = 1;
            for (int64_t q = c0 / B; q <= (c1 - 1) / B; ++q) {
                if (q * B == lo) continue;                               // the own block is there already
                const int64_t off_hi = ((c1 < (q + 1) * B) ? c1 : (q + 1) * B) - 1 - q * B;
                int c = 0;
                while (c + 1 < C && s.sb[c + 1] <= off_hi) ++c;
                if (1 + c > ph) ph = 1 + c;
            }
        }
        phase[(size_t)p] = ph;
        ++cnt[ph];
    }
    // Slots.  Measured on shard-shaped matrices with a spin kernel standing in for the gather (tools/split_timing.py):
    // each launch must fit ONE round of workgroups (2 per CU) or its tail costs more than the overlap gains; the
    // other panels take as many groups as fit; the local panels enough groups that a workgroup walks <= ~13 panels
    // and is done by the time the gather is.  10M x 10M: 8 ranks (2 + 8 groups) 0.402 -> 0.380 ms per half-step,
    // 4 ranks (3 + 4) 0.677 -> 0.573 ms, 2 ranks (2 + 2) 1.27 -> 1.01 ms.
    const int round_slots = 2 * 256;
    int fit = round_slots / (s.t.nblk > 0 ? s.t.nblk : 1);
    fit = fit < 1 ? 1 : fit;
    // Group counts are powers of two: the group is the fast index of blockIdx and workgroups are dealt round-robin over the 8 XCDs,
    // so with 8 (16) groups each XCD's L2 holds the panels of one (two) groups only, with 2 or 4 groups of two or four -- any other
    // count spreads every group over all XCDs and each of them pulls the whole gathered vector (measured: k_tiled_fused).
    auto pow2 = [](int g) { int p = 1; while (2 * p <= g) p *= 2; return p; };
    auto norm = [&](int g, int n) { if (n <= 0) return 0; g = g < 1 ? 1 : (g > n ? n : g); return pow2(g); };
    int a = (nloc + 12) / 13;
    a = a > fit ? fit : a;
    a = a > nloc ? nloc : a;
    int g[MAX_PHASE] = {0};
    if (C == 1) {
        int b = fit < nrem ? fit : nrem;
        if (a + b > h->rs_groups) b = h->rs_groups - a;
        if (a < 1 || b < 1) return PDLP_OK;
        int S = a + b;
        if (h->split_local >= 1 && h->split_other >= 1 && h->split_local + h->split_other <= h->rs_groups) {   // PDLP_OPT_SPLIT_SLOTS (tools)
            a = h->split_local;
            S = h->split_local + h->split_other;
        }
        g[0] = norm(a, nloc);
        g[1] = norm(S - a, nrem);
    } else {
        // every chunk's launch fills the chip by itself where it can; fewer groups per chunk when the scratch runs out
        int left = h->rs_groups - a;
        if (a < 1 || left < C) return PDLP_OK;
        g[0] = norm(a, nloc);
        int want[MAX_PHASE] = {0}, sum = 0;
        // (the last phase of a product whose result travels in pieces is launched piece by piece: each launch covers only nb_max row
        //  blocks and needs proportionally more groups to fill the chip)
        int fit_last = R > 1 && nb_max > 0 ? round_slots / nb_max : fit;     // (the phase's own group count left the chip half empty: 0.92 against 0.81 ms per iteration at 8 ranks)
        fit_last = fit_last < 1 ? 1 : fit_last;
        for (int c = 0; c < C; ++c) {
            const int f = c == C - 1 ? fit_last : fit;
            want[1 + c] = cnt[1 + c] > 0 ? (f < cnt[1 + c] ? f : cnt[1 + c]) : 0;
            sum += want[1 + c];
        }
        for (int c = 0; c < C; ++c) {
            int w = want[1 + c];
            if (sum > left && w > 0) { w = (int)((int64_t)w * left / sum); w = w < 1 ? 1 : w; }
            g[1 + c] = norm(w, cnt[1 + c]);
        }
    }
    // the table: panels phase by phase, ascending inside a phase
    std::vector<int32_t> tab((size_t)npanel);
    int off = 0, slot = 0;
    s.nphase = 1 + C;
    for (int ph = 0; ph < s.nphase; ++ph) {
        s.ph_off[ph] = off; s.ph_cnt[ph] = cnt[ph]; s.ph_slots[ph] = g[ph]; s.ph_slot0[ph] = slot;
        for (int p = 0; p < npanel; ++p)
            if (phase[(size_t)p] == ph) tab[(size_t)off++] = p;
        slot += g[ph];
    }
    if (slot > h->rs_groups) { s.nphase = 0; return PDLP_OK; }
    HIP_TRY(hipMemcpyAsync(s.ptab, tab.data(), (size_t)npanel * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));                          // (the host vector goes away)
    s.loc_pa = pa; s.loc_pb = pb;
    s.slotsA = g[0];
    s.slotsB = slot - g[0];
    s.nrange = (R > 1 && C > 1) ? R : 0;          // (one exchange piece = one all-gather: nothing to send early)
    return PDLP_OK;
}

// after a change of what the plan depends on (exchange chunks, producer pieces, slot counts): both products' plans anew
int reconfigure_splits(pdlp_handle h)
{
    drop_graphs(h);               // captured launches name the old plan
    const int rc = configure_split(h, false);
    return rc == PDLP_OK ? configure_split(h, true) : rc;
}

}  // namespace
