// pdlp_handle.inc -- what a solver handle is made of: Schedule (the state of one matrix's product), Carried (which carried product
// still belongs to its vector, with the transitions that are its only writers), struct pdlp_solver (every field initialised at its
// declaration), the workspace Layout with the capacities derived from the problem's sizes, and the functions that check a problem,
// bind a handle to its workspace and release it.
// Part of pdlp_hip.hip (included at file scope; not a translation unit of its own).  Needs: the constants, HIP_TRY, align_up
// (pdlp_hip.hip), TNT / TRPT_MAX_ANY (pdlp_kernel_tiled.inc), g_rccl (pdlp_loaders.inc).
// ------------------------------------------------------------------------------------------------
namespace {

struct Schedule {
    int64_t* blk = nullptr;   // device, nblk+1 pairs (first row, first non-zero)
    uint32_t* rplo = nullptr; // device, rows+1: the LOW 32 bits of the row pointers.  Inside a row block the kernel only needs offsets relative
                              // to the block's first non-zero (< 2^32 apart), so it reads 4 bytes per row instead of 8: (uint32)(rp[r]) - (uint32)a
    int nblk = 0;
    int grid = 0;
    // rows longer than NNZ_CAP, cut into chunks of NNZ_CAP non-zeros
    int64_t* lch = nullptr;   // device, [2*nchunks] (first, end) non-zero of every chunk
    int32_t* lrow = nullptr;  // device, [nlong] the rows
    int32_t* lptr = nullptr;  // device, [nlong+1] their chunk ranges
    void* longpart = nullptr; // device, [nchunks] chunk sums
    int nchunks = 0, nlong = 0, lgrid = 0;
    // column-sorted row blocks (optional, attached by the caller): the CSR kernel reads each block's items sorted by column
    const uint32_t* sidx = nullptr;
    const void* sval = nullptr;
    const int32_t* cbase = nullptr;
    // panel-tiled copy (optional, attached by the caller): used instead of the CSR arrays when set
    bool tiled = false;
    pdlp_tiles t{};
    // the tile set's packed index stream (pdlp_attach_packed_items: float32 handles; null = the kernel reads t.idx)
    const uint32_t* idx24 = nullptr;
    const uint32_t* run_base = nullptr;
    // sharded problems: the panels lying wholly inside the locally owned block of the gathered vector, [loc_pa, loc_pb),
    // can be multiplied before the all-gather of that vector has finished (pdlp_*_half_begin)
    int loc_pa = 0, loc_pb = 0;
    int slotsA = 0, slotsB = 0;   // panel groups (= partial row sum slots) of the local and of all the other panels
    bool pending = false;         // the local panels of the next product are already in rowsum[0 .. slotsA)
    bool pending_inline = false;  // ... and were launched on the handle's own stream (PDLP_OPT_BEGIN_INLINE): nothing to join
    // the exchange of the gathered vector in `nphase - 1` chunks (pdlp_set_exchange_chunks): chunk c moves elements
    // [sb[c], sb[c+1]) of EVERY rank's block; a panel belongs to the phase with which its last foreign entry arrives
    // (phase 0: the panels of the own block, phase 1 + c: chunk c).  ptab holds the panels phase by phase.
    int32_t* ptab = nullptr;      // device, room for every panel of the matrix
    int64_t ptab_cap = 0;
    int nphase = 0;               // 0: product not split
    int ph_off[MAX_PHASE] = {0}, ph_cnt[MAX_PHASE] = {0}, ph_slots[MAX_PHASE] = {0}, ph_slot0[MAX_PHASE] = {0};
    int64_t sb[MAX_PHASE] = {0};
    int chunks_done = 0;          // chunk phases of the pending product already launched (pdlp_half_chunk)
    // the RESULT of the product travels in `nrange` pieces (the plan of the exchange that follows): piece r = the rows of the row
    // blocks [rb_lo[r], rb_lo[r+1]); the last phase and the epilogue of a split product then run piece by piece (launch_mat)
    int nrange = 0;
    int rb_lo[MAX_PHASE] = {0};
};

// upper bound on the number of row blocks: two consecutive blocks together exceed a cap
inline int64_t max_blocks(int64_t rows, int64_t nnz) { return 2 * (rows / ROWS_CAP + nnz / NNZ_CAP) + 4; }

// upper bounds on the chunks / long rows of a matrix with nnz non-zeros
inline int64_t max_chunks(int64_t nnz) { return 2 * (nnz / NNZ_CAP) + 2; }
inline int64_t max_long(int64_t nnz) { return nnz / NNZ_CAP + 1; }
constexpr int LONG_GRID = 64;

// panel groups the row-sum scratch is sized for: splitting only pays when one workgroup per (largest) row block
// cannot fill 2 x 256 CUs, i.e. below about 10.5M rows
inline int64_t rowsum_groups(int64_t rows)
{
    if (rows <= (int64_t)512 * 40 * 128) return 32;               // (small shards: room for the local panels and several chunks' groups)
    return rows <= (int64_t)512 * 40 * 512 ? 8 : 1;
}

// What the single-LP handle carries so as not to multiply again, and whether each carried product still belongs to its vector.
// THE RULES ARE WRITTEN HERE AND NOWHERE ELSE: a field says which buffer it speaks about, which vector that buffer must belong to
// for the field to be up, and which events raise and clear it.  The member functions below are those events and the ONLY writers;
// everything else reads the fields.  Plain and copyable: pair_graph copies the whole struct around a capture.  The option switches
// (no_running, no_kty_reuse, graph_ok, delta) are configuration and stay in pdlp_solver; a transition that depends on one takes it.
enum { CAND_NONE = 0, CAND_KX_OWN, CAND_KX_CARRIED };
struct Carried {
    // kxb[0] is K x of the CURRENT x (delta mode: the float64 anchor K x_cur).  Up: a K x refresh, exact or given anchors, a
    // restart that adopted a candidate WITH products.  Down: a restart without them (also to the current iterate: the next dual
    // half-step multiplies once), a discarded trial (kxb[0] belongs to the rejected x+), Halpern iterations, a mode switch.  Every
    // dual half-step keeps it up by carrying kxb[0] along.
    bool kx_valid = false;
    // The KKT pass of the CURRENT iterate kept K'y_cur in ktyb[0] and K x_cur in kxb[1] (CAND_KX_OWN: it multiplied) or took K x from
    // kxb[0] (CAND_KX_CARRIED: nothing to swap on a restart; always this in delta mode).  Up: kkt_kept(PDLP_CUR).  Down: whatever
    // moves the current iterate or changes the operands -- an iteration, a restart, new operands, drop_products.  (One field where
    // there were two, cand_valid[0] and cur_kx_cached: the second was read only under the first, and every pass that raised the
    // first set the second.)
    int cand_cur = CAND_NONE;
    // The KKT pass of the AVERAGED iterate (the Halpern candidate) kept K'y in ktyb[1] and K x in kxb[2]; same events.
    bool cand_avg = false;
    // ktyb[kty_cur] is K'y of the CURRENT y although cand_cur is down: the restart adopted candidate kty_cur with its products.
    // -1: none (see cand_cur).  Up: restart_adopted with products.  Down: an iteration; a KKT pass at the current iterate (its own
    // copy in ktyb[0] supersedes) or one that overwrites ktyb[1] while that is the copy; an average formed into ktyb[1]; a restart
    // to the average without products; new operands; drop_products.
    int kty_cur = -1;
    // Delta mode: kxb[0] / ktyr are the float64 anchors of the current iterate (anchors_valid), and ktyr is K'y of the CURRENT y
    // (dy_folded; else of the previous y, with gdy = y_cur - y_prev still to be folded in by the next product with K').  Both false
    // outside delta mode.  Up: anchors_exact / anchors_given, folded; a restart to the average that adopted its products.  Down:
    // dy_folded by an iteration; anchors_valid by a restart to the average without products; both by drop_products.
    bool anchors_valid = false, dy_folded = false;
    // Iterations since kx_sum / kty_sum (and x_sum, y_sum, eta_sum) were last zeroed; also the Halpern count t.  Not counted in
    // delta mode, which keeps no running products.  Up: iterated -- replays of captured pairs included: a replay touches no host
    // state, so replayed() counts for it.  Down: one by trial_undone; zero by period_reset.
    int64_t since_reset = 0;
    // kty_sum already holds the term of the CURRENT y (the fixed step adds the term of an iterate one half-step late; the flush at a
    // restart check adds it at once).  Up: flushed_tail.  Down: an iteration, period_reset.  Read only while sums_broken is down.
    bool kty_tail_done = false;
    // kx_sum / kty_sum miss a term of this period, or hold one with another weight than x_sum / y_sum: no product of the average
    // from the sums, the checks multiply.  Up: sums_end inside a period (the callers say why), a discarded trial, Halpern iterations.
    // Down: period_reset, which goes with the zeroing of the sums.
    bool sums_broken = false;
    // kxb[2] / ktyb[1] are K x_avg / K'y_avg of the average in the PDLP_AVG buffers, formed from the sums.  Up: averaged(true).
    // Down: averaged(false), period_reset, drop_all -- and an iteration, as a safeguard: nothing an iteration writes is read under
    // this flag (profiles/r13_sequences/README.md, mutant (a)).
    bool avg_products = false;
    // pdlp_halpern_iterate has run since the last pdlp_set_iterate: PDLP_AVG holds its candidate, not an average, and the two
    // averaging calls are refused.  Up: halpern_begins.  Down: new_iterate only.
    bool halpern = false;
    // PDLP_PREV / PDLP_AVG are still z / T(z) of the last Halpern iteration (pdlp_halpern_fixed_point).  Up: halpern_begins.
    // Down: buffers_reassigned -- any call that re-assigns the iterate buffers.
    bool halpern_pair = false;
    // Sparse quadratic objective: lam_prev is c + Q x of the CURRENT x, so the adaptive iteration (pdlp_objective_iterate) need not
    // form it ahead of its primal half-step.  Up: gradient_stepped -- the step product of that iteration, which multiplies at the x'
    // the dual half-step of the same iteration then makes current (a rejected trial is kept: x' stays); raised only once that
    // half-step has swapped the buffers, and down from the moment the product overwrites the buffer (an iteration that fails in
    // between leaves it down).  Down: whatever else writes lam_prev or moves x -- a KKT pass or report at any point
    // (gradient_overwritten: it forms g of the point it looks at, the current one included), the fixed primal half-step (it forms g
    // of the x it then leaves), every finished iteration (iterated: any dual half-step swaps the buffers, a bare pdlp_dual_half
    // included), a restart, new_iterate, objective_matrix_changed, drop_all.  Read by pdlp_objective_iterate alone: the fixed-step path forms g ahead of every primal
    // half-step whatever this says.
    bool g_cur = false;

    // A capture (pair_graph) runs the launch code, transitions included, and puts the whole struct back: it leaves no trace.  It used
    // to restore kx_valid, the candidates, since_reset and kty_tail_done only; what it left in the others, and why replayed() gives
    // every later call the same answer: kty_cur = -1 and avg_products = false as after an iteration -- replayed() IS iterated();
    // sums_broken, halpern and halpern_pair as they were (no half-step writes the first two, pdlp_iterate had cleared the third);
    // delta mode: anchors_valid up (a capture starts only with kx_valid up, which the anchors raise together with it) and dy_folded
    // down as after an iteration -- iterated() again.  A replay from a CACHED graph used to leave kty_cur and avg_products alone,
    // stale after a restart; under replay nothing reads them, and replayed() now clears them before replay can be switched off.

    void new_iterate() { *this = Carried(); }                                  // pdlp_set_iterate: nothing belongs to the new vectors
    void period_reset() { since_reset = 0; kty_tail_done = avg_products = sums_broken = false; }     // the sums were zeroed
    void drop_candidates() { cand_cur = CAND_NONE; cand_avg = false; }
    // pdlp_restart made candidate `cand` (0: current, 1: average) the current iterate, with the products its KKT pass had left or
    // without (the caller swaps the buffers BEFORE this call: it reads the candidates).  Delta mode keeps no running sums: no period.
    void restart_adopted(int cand, bool delta)
    {
        const bool had = cand == 0 ? cand_cur != CAND_NONE : cand_avg;
        if (delta) {
            if (cand == 1) { if (had) dy_folded = true; else anchors_valid = false; }
        } else {
            kx_valid = had;
            if (had) kty_cur = cand; else if (cand == 1) kty_cur = -1;
            period_reset();
        }
        drop_candidates();
        g_cur = false;
    }
    // `n` PDHG iterations finished (the last dual half-step of each has swapped the buffers)
    void iterated(int64_t n, bool delta)
    {
        if (delta) dy_folded = false;      // gdy = y_cur - y_prev waits for the next product with K'
        else { since_reset += n; kty_tail_done = avg_products = false; kty_cur = -1; }
        drop_candidates();
        g_cur = false;          // (x has moved; pdlp_objective_iterate raises it again behind its own dual half-step)
    }
    void replayed(int pairs, bool delta) { iterated(2 * (int64_t)pairs, delta); }      // `pairs` launches of a captured pair
    // a KKT pass at `which` is about to overwrite its K'y slot / has kept its products (kx_carried: K x came from kxb[0])
    void kkt_begins(int which) { if (which == PDLP_CUR || (which == PDLP_AVG && kty_cur == 1)) kty_cur = -1; }
    void kkt_kept(int which, bool kx_carried)
    {
        if (which == PDLP_CUR) cand_cur = kx_carried ? CAND_KX_CARRIED : CAND_KX_OWN;
        if (which == PDLP_AVG) cand_avg = true;
    }
    void averaged(bool from_sums) { avg_products = from_sums; if (from_sums && kty_cur == 1) kty_cur = -1; }
    void flushed_tail() { kty_tail_done = true; }
    // the running sums stop being complete inside a period (at since_reset == 0 nothing has been added yet: nothing is missing)
    void sums_end() { if (since_reset > 0) sums_broken = true; }
    void operands_changed() { drop_candidates(); kty_cur = -1; }               // what a KKT pass kept belongs to the other q_upper / d
    // pdlp_set_objective_matrix: Q set, replaced or taken away.  What a KKT pass kept goes, as with the other operands of the
    // objective, and the gradient buffer g = c + Q x belongs to the other Q (the fixed step never carries it: every primal half-step
    // and every KKT pass forms it anew; see g_cur)
    void objective_matrix_changed() { operands_changed(); g_cur = false; }
    void gradient_stepped() { g_cur = true; }                                  // lam_prev = c + Q x' and x' has just become current
    void gradient_overwritten() { g_cur = false; }                             // a KKT pass, a report, the fixed primal half-step
    // pdlp_set_delta: no product survives the switch.  The sums' fields stay as they are, as they always did: delta mode reads none.
    void drop_products() { kx_valid = false; drop_candidates(); kty_cur = -1; anchors_valid = dy_folded = false; }
    // nothing carried survives, the running sums of this period included.  (One list where pdlp_halpern_iterate and
    // pdlp_adaptive_retry had two that differed in cur_kx_cached: see cand_cur.  Neither runs in delta mode: the anchors are down.)
    void drop_all() { drop_products(); kty_tail_done = avg_products = false; sums_broken = true; g_cur = false; }
    void trial_undone() { if (since_reset > 0) --since_reset; drop_all(); }    // pdlp_adaptive_retry: the products saw the rejected trial
    void halpern_begins() { drop_all(); halpern = halpern_pair = true; }       // (every primal half of the mode multiplies)
    void halpern_iterated() { ++since_reset; }
    void buffers_reassigned() { halpern_pair = false; }
    void kx_refreshed() { kx_valid = true; }
    void anchors_exact() { anchors_valid = dy_folded = kx_valid = true; }      // delta_refresh
    void anchors_given() { anchors_exact(); drop_candidates(); }               // pdlp_set_anchors
    void folded() { dy_folded = true; }                                        // ktyr now belongs to the current y
};

}  // namespace

// Every field carries its initial value HERE; pdlp_create sets only what depends on the problem (p, stream, es, mixed, nl, ml,
// ineq_end) and bind_layout the pointers into the workspace.
struct pdlp_solver {
    pdlp_problem p{};
    hipStream_t stream = nullptr;
    size_t es = 0;                // element size of the vectors
    bool mixed = false;           // PDLP_MIXED: float32 matrix values under float64 vectors
    // delta mode (mixed precision only): every product of the iteration runs on the float32 kernels over a float32 DIFFERENCE
    // vector and is added to a float64 "anchor" product that is carried along: kxb[0] = K x_cur, ktyr = K'y (Carried: anchors_valid,
    // dy_folded)
    bool delta = false;
    ncclComm_t comm = nullptr;    // RCCL communicator of a sharded problem (pdlp_comm_init), or null: the caller does the exchange
    int comm_rank = 0, comm_size = 1;
    int xchunks = 1;              // chunks of the exchange of a gathered vector (pdlp_set_exchange_chunks); 1: one all-gather
    hipStream_t cstream = nullptr;  // the chunks travel on this stream while the handle's stream multiplies what has arrived
    hipEvent_t ev_vec = nullptr, ev_chunk[MAX_CHUNKS] = {};
    hipEvent_t ev_ar = nullptr;     // library driver: the step-size rule's all-reduce on the communication stream has finished
    hipEvent_t ev_row[MAX_CHUNKS] = {};  // library driver: piece r of the vector a half-step is producing is final on the handle's stream
    int range_sel = -1, range_cnt = 1;   // >= 0: the half-step being issued covers only output piece `range_sel` of `range_cnt` (pdlp_*_half_piece)
    char* ktyr = nullptr;         // [nl] float64 running K'y
    float *gdx = nullptr, *gdy = nullptr;   // full-length float32 difference vectors the float32 kernels gather from
    int64_t nl = 0, ml = 0;       // local variable / constraint counts
    int ineq_end = 0;             // local rows below this index are inequalities
    const void* obj_diag = nullptr;  // diagonal quadratic objective (pdlp_set_objective_diag): c'x + 1/2 x'Dx, d of the variables; the caller's memory
    const void* q_upper = nullptr;   // two-sided rows (pdlp_set_row_upper): q <= K x <= q_upper on the inequality rows; the caller's memory
    // sparse quadratic objective (pdlp_set_objective_matrix): c'x + 1/2 x'Qx.  Q's CSR arrays are the caller's memory; sQ is its
    // row-block schedule, built into the caller's `work`; the gradient g = c + Q x of the point a half-step or a KKT pass looks at
    // lives in lam_prev (the infeasibility detector's, which is refused while Q is set); red[OBJ_XQX] receives x'Qx of a KKT pass;
    // part: the partial sums of the step product's curvature (pdlp_objective_iterate), at the end of the caller's `work`
    struct ObjMatrix { bool on = false; const int32_t* colidx = nullptr; const void* val = nullptr; double* part = nullptr; } obj_mat;
    static constexpr int OBJ_XQX = PDLP_NRED - 1;
    Schedule sK, sKT, sQ;
    char* xb[3] = {};             // full-length primal buffers; roles via ix_*
    char* yb[3] = {};
    int ix_cur = 0, ix_prev = 1, ix_avg = 2;  // (x and y rotate together)
    char* xbar = nullptr;
    char *x_sum = nullptr, *y_sum = nullptr, *x_last = nullptr, *y_last = nullptr;
    char* kxb[3] = {};            // K x caches: [0] running, [1] from KKT(cur), [2] from KKT(avg)
    char *dxf = nullptr, *dyf = nullptr;         // infeasibility detection: full-length x - x_prev, y - y_prev (gathered by the caller when sharded)
    char *lam_prev = nullptr, *ktdy = nullptr;   //   this rank's block of the previous lambda and of K'dy
    char* ktyb[2] = {};           // K'y of the candidates, kept by their KKT passes: [0] current, [1] averaged iterate
    Carried carry;                // which carried product still belongs to its vector
    bool no_kty_reuse = false;    // PDLP_OPT_KTY_REUSE = 0: timing experiments
    int split_local = 0, split_other = 0;   // PDLP_OPT_SPLIT_SLOTS: panel groups of a split product chosen by the caller (0: the library's rule)
    bool side_ok = false;         // the library's own streams and events exist (graph replay, split products)
    bool begin_inline = false;    // PDLP_OPT_BEGIN_INLINE: pdlp_*_half_begin launch on the handle's stream (the caller's exchange is asynchronous)
    bool producer_pieces = true;  // PDLP_OPT_PRODUCER_PIECES (default on): results of split products leave piece by piece (Schedule::nrange)
    char* ws = nullptr;           // the caller's workspace (pdlp_peer_export hands it to the other ranks)
    int64_t ws_bytes = 0;
    // direct exchange (pdlp_peer_*): the other ranks' workspaces and mailboxes, opened over HIP IPC
    struct Peer {
        bool on = false;          // connected
        bool enabled = true;      // PDLP_OPT_PEER_EXCHANGE: pdlp_iterate uses it
        bool active = false;      // inside iterate_peer: the half-steps' epilogues store into the peers
        bool loopback = false;    // timing stand-in: the "peers" are scratch buffers of this process
        bool local_first = false; // PDLP_OPT_PEER_LOCAL_FIRST: the own block's panels are multiplied between signal and wait
        bool push = false;        // PDLP_OPT_PEER_PUSH: the block leaves by a copy kernel on the side stream, beside those panels
        int rank = 0, world = 1, n = 0;      // n = world - 1 peers
        void* opened[2 * MAX_PEER] = {};     // what hipIpcCloseMemHandle wants back
        int nopened = 0;
        char* out[6][MAX_PEER] = {};         // peer i's xbar, y buffers 0 / 1 / 2, gdx, gdy -- at THIS rank's block
        uint32_t* flag[MAX_PEER] = {};       // this rank's slot in peer i's mailbox
        double* sums[MAX_PEER] = {};
        char* box = nullptr;                 // the own mailbox (fine-grained device memory)
        char* scratch = nullptr;             // loopback: the stand-in destinations
        char* scratch_host = nullptr;        // PDLP_PEER_LOOPBACK_HOST: one of them in pinned host memory (a slow link's stand-in)
        hipStream_t pstream = nullptr;       // push form: a HIGH-priority stream -- the copy kernel must get its few waves onto the
        hipEvent_t ev_push = nullptr;        //   chip before the own-block panels' launch fills every CU's registers
        int* err = nullptr;                  // host memory the wait kernel reports a timeout through
        int* err_dev = nullptr;
        uint32_t seq = 0;
        long long limit_ticks = 1000000000LL;   // 10 s of the 100 MHz clock
    } peer;
    // running products: K x (kxb[0]) is carried along by every dual half-step and both products are summed with the
    // average's weights (kx_sum, kty_sum), so a restart check evaluates K x_cur, K x_avg and K'y_avg WITHOUT products:
    // one product (K'y_cur, kept for the next primal half-step) instead of four per check
    char *kx_sum = nullptr, *kty_sum = nullptr;
    bool no_running = false;      // PDLP_OPT_RUNNING_KKT = 0: every KKT pass multiplies (round-1 behaviour)
    double *partA = nullptr, *partB = nullptr, *red = nullptr, *sc = nullptr;
    void* rowsum = nullptr;       // row sums of the tiled kernel on their way to the epilogue: [groups][rs_stride]
    int64_t rs_stride = 0;        // rows + one row block                        (these three: copied from the Layout)
    int rs_groups = 0;            // panel groups the scratch has room for
    int64_t part_blocks = 0;      // workgroups partA / partB have room for
    int last_gridA = 0, last_gridB = 0;   // grids of the last primal / dual launch (adaptive reduce)
    bool use_split = false;       // set by the half-step that may consume a pending local-panel product
    // optional (PDLP_OPT_GRAPH): pdlp_iterate replays two captured iterations (the buffer roles return after two) as one
    // hipGraph launch.  Captured on and replayed from the library's own stream (capture is not allowed on the
    // legacy null stream), ordered against the caller's stream with events.  One graph per (roles, mode).
    hipStream_t gstream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    bool graph_ok = false;        // pdlp_set_option(PDLP_OPT_GRAPH) turns the replay on
    struct IterGraph { bool valid = false; int ix_cur = 0, ix_prev = 0, adaptive = 0; hipGraphExec_t exec = nullptr; } graphs[12];
    // batched solves with a matrix per LP (optional, attached by the caller: pdlp_batch_attach_matrices): the values of K and K'
    // as populations [nnz][Bp] over the handle's pattern, the Ruiz factors as [n][Bp] / [m][Bp]; used by every pdlp_batch_* call
    struct BatchMatrices { int Bp = 0; const void *K_val = nullptr, *KT_val = nullptr, *d_col = nullptr, *d_row = nullptr; } bm;
    int64_t nnz = 0;           // stored entries of K (the rows of a value population: pdlp_batch_admit)
};

namespace {

// what the PDLP_ERR_STATE guards of the entry points ask of a handle
inline bool whole_problem(pdlp_handle h) { return h->nl == h->p.n && h->ml == h->p.m; }        // all of the LP on this GPU, not a shard
inline bool plain_single(pdlp_handle h)         // ... in one precision and outside every exchange: the only form the extensions have
{
    return whole_problem(h) && !h->mixed && !h->delta && !h->comm && !h->peer.on;
}
inline bool has_extension(pdlp_handle h) { return h->q_upper || h->obj_diag || h->obj_mat.on; }    // two-sided rows or a quadratic objective
inline bool mid_split_product(pdlp_handle h) { return h->sK.pending || h->sKT.pending; }      // in the middle of a split product

void drop_graphs(pdlp_handle h)
{
    for (auto& g : h->graphs) {
        if (g.valid) (void)hipGraphExecDestroy(g.exec);
        g.valid = false;
    }
}

// the direct exchange's mappings and allocations (the peers' memory is only unmapped here, never freed)
void peer_release(pdlp_handle h)
{
    pdlp_solver::Peer& P = h->peer;
    for (int i = 0; i < P.nopened; ++i) if (P.opened[i]) (void)hipIpcCloseMemHandle(P.opened[i]);
    if (P.box) (void)hipFree(P.box);
    if (P.scratch) (void)hipFree(P.scratch);
    if (P.scratch_host) (void)hipHostFree(P.scratch_host);
    if (P.pstream) { (void)hipStreamSynchronize(P.pstream); (void)hipStreamDestroy(P.pstream); }
    if (P.ev_push) (void)hipEventDestroy(P.ev_push);
    if (P.err) (void)hipHostFree(P.err);
    (void)hipGetLastError();
    P = pdlp_solver::Peer();
}

void free_handle(pdlp_handle h)
{
    drop_graphs(h);
    if (h->comm && g_rccl.CommDestroy) { (void)g_rccl.CommDestroy(h->comm); h->comm = nullptr; }
    if (h->gstream) { (void)hipStreamSynchronize(h->gstream); (void)hipStreamDestroy(h->gstream); }
    if (h->cstream) { (void)hipStreamSynchronize(h->cstream); (void)hipStreamDestroy(h->cstream); }
    if (h->ev_vec) (void)hipEventDestroy(h->ev_vec);
    for (auto& e : h->ev_chunk) if (e) (void)hipEventDestroy(e);
    for (auto& e : h->ev_row) if (e) (void)hipEventDestroy(e);
    if (h->ev_ar) (void)hipEventDestroy(h->ev_ar);
    if (h->ev_in) (void)hipEventDestroy(h->ev_in);
    if (h->ev_out) (void)hipEventDestroy(h->ev_out);
    peer_release(h);
    delete h;
}

int check_problem(const pdlp_problem* p)
{
    if (!p) return PDLP_ERR_INVALID;
    if (p->dtype != PDLP_F32 && p->dtype != PDLP_F64 && p->dtype != PDLP_MIXED) return PDLP_ERR_INVALID;
    if (p->m < 0 || p->n < 0 || p->m_ineq < 0 || p->m_ineq > p->m) return PDLP_ERR_INVALID;
    if (p->row0 < 0 || p->row1 < p->row0 || p->row1 > p->m) return PDLP_ERR_INVALID;
    if (p->col0 < 0 || p->col1 < p->col0 || p->col1 > p->n) return PDLP_ERR_INVALID;
    if (p->m >= INT32_MAX || p->n >= INT32_MAX) return PDLP_ERR_INVALID;
    return PDLP_OK;
}

struct Carve {
    int64_t off = 0;
    int64_t take(int64_t bytes) { const int64_t o = off; off = align_up(off + bytes, 256); return o; }
};

// The caller's workspace: byte offsets of everything the handle keeps in it, IN THE ORDER OF THE MEMBERS (256-byte aligned), and
// the capacities derived from the problem's sizes.  Filled by layout() alone, for the size query and for pdlp_create; a new buffer
// is a new member here, a take() at its place in layout() and a pointer in bind_layout().  pdlp_create zeroes [xb[0], sched[0])
// and [dxf, rplo[0]): a buffer whose initial contents must be zero goes into one of these two stretches.
struct Layout {
    int64_t xb[3], yb[3], xbar, x_sum, y_sum, x_last, y_last;
    int64_t kxb[3];                       // K x caches
    int64_t partA, partB, red, sc;
    int64_t sched[2];                     // row-block schedules of K, K' (pairs of 64-bit words)
    int64_t rowsum;                       // row-sum scratch of the tiled kernel
    struct LongRows { int64_t lch, lrow, lptr, longpart; } long_rows[2];   // rows longer than NNZ_CAP of K, K'
    int64_t dxf, dyf, lam_prev, ktdy;     // infeasibility detection
    int64_t ktyb[2];                      // K'y from KKT(current), KKT(average)
    int64_t ktyr, gdx, gdy;               // delta mode (mixed precision only, else empty)
    int64_t kx_sum, kty_sum;              // running sums of w_k K x_k, w_k K'y_k
    int64_t ptab[2];                      // panels by phase of K, K' (sharded problems only, else empty)
    int64_t rplo[2];                      // low words of the row pointers of K, K' (the CSR kernel's 4-byte reads)
    int64_t bytes;                        // the whole workspace
    // capacities
    int64_t part_blocks;                  // workgroups partA / partB have room for: the CSR grid (+ long rows), one workgroup per >= 512
                                          // rows (tiled, rpt >= 1), or the epilogue launches of up to MAX_CHUNKS output pieces
    int64_t rs_stride;                    // row-sum scratch: elements per panel group (rows + one row block) ...
    int rs_groups;                        // ... and panel groups
    bool sharded;
    int64_t ptab_cap[2];                  // panels a table has room for (panel width >= 16 columns)
};

Layout layout(const pdlp_problem* p, int64_t nnzK, int64_t nnzKT)
{
    const int64_t es = p->dtype == PDLP_F32 ? 4 : 8;
    const int64_t nl = p->col1 - p->col0, ml = p->row1 - p->row0, rmax = nl > ml ? nl : ml;
    const bool mixed = p->dtype == PDLP_MIXED;
    Layout L{};
    L.part_blocks = (int64_t)MAX_GRID * MAX_CHUNKS + LONG_GRID + rmax / TNT + 2;
    L.rs_stride = rmax + (int64_t)TNT * TRPT_MAX_ANY;
    L.rs_groups = (int)rowsum_groups(rmax);
    L.sharded = nl != p->n || ml != p->m;
    L.ptab_cap[0] = (p->n >> 4) + 8;
    L.ptab_cap[1] = (p->m >> 4) + 8;
    Carve c;
    for (auto& o : L.xb) o = c.take(p->n * es);
    for (auto& o : L.yb) o = c.take(p->m * es);
    L.xbar = c.take(p->n * es);
    L.x_sum = c.take(nl * es);
    L.y_sum = c.take(ml * es);
    L.x_last = c.take(nl * es);
    L.y_last = c.take(ml * es);
    for (auto& o : L.kxb) o = c.take(ml * es);
    L.partA = c.take(L.part_blocks * NACC * 8);
    L.partB = c.take(L.part_blocks * NACC * 8);
    L.red = c.take(PDLP_NRED * 8);
    L.sc = c.take(PDLP_NSCAL * 8);
    L.sched[0] = c.take((max_blocks(ml, nnzK) + 1) * 16);
    L.sched[1] = c.take((max_blocks(nl, nnzKT) + 1) * 16);
    L.rowsum = c.take(L.rs_groups * L.rs_stride * es);
    for (int t = 0; t < 2; ++t) {
        const int64_t nnz = t == 0 ? nnzK : nnzKT;
        L.long_rows[t].lch = c.take(max_chunks(nnz) * 2 * 8);          // chunk (first, end), 64-bit
        L.long_rows[t].lrow = c.take(max_long(nnz) * 4);               // rows
        L.long_rows[t].lptr = c.take((max_long(nnz) + 1) * 4);         // chunk ranges
        L.long_rows[t].longpart = c.take(max_chunks(nnz) * es);        // chunk sums
    }
    L.dxf = c.take(p->n * es);
    L.dyf = c.take(p->m * es);
    L.lam_prev = c.take(nl * es);
    L.ktdy = c.take(nl * es);
    for (auto& o : L.ktyb) o = c.take(nl * es);
    L.ktyr = c.take(mixed ? nl * es : 0);
    L.gdx = c.take(mixed ? p->n * 4 : 0);
    L.gdy = c.take(mixed ? p->m * 4 : 0);
    L.kx_sum = c.take(ml * es);
    L.kty_sum = c.take(nl * es);
    for (int t = 0; t < 2; ++t) L.ptab[t] = c.take(L.sharded ? L.ptab_cap[t] * 4 : 0);
    L.rplo[0] = c.take((ml + 1) * 4);
    L.rplo[1] = c.take((nl + 1) * 4);
    L.bytes = c.off;
    return L;
}

// the handle's pointers into the workspace `w` and the capacities it checks against
void bind_layout(pdlp_handle h, char* w, const Layout& L)
{
    h->ws = w; h->ws_bytes = L.bytes;
    for (int i = 0; i < 3; ++i) { h->xb[i] = w + L.xb[i]; h->yb[i] = w + L.yb[i]; h->kxb[i] = w + L.kxb[i]; }
    h->xbar = w + L.xbar;
    h->x_sum = w + L.x_sum; h->y_sum = w + L.y_sum; h->x_last = w + L.x_last; h->y_last = w + L.y_last;
    h->partA = (double*)(w + L.partA); h->partB = (double*)(w + L.partB);
    h->red = (double*)(w + L.red); h->sc = (double*)(w + L.sc);
    h->rowsum = (void*)(w + L.rowsum);
    h->dxf = w + L.dxf; h->dyf = w + L.dyf; h->lam_prev = w + L.lam_prev; h->ktdy = w + L.ktdy;
    h->ktyb[0] = w + L.ktyb[0]; h->ktyb[1] = w + L.ktyb[1];
    h->ktyr = w + L.ktyr; h->gdx = (float*)(w + L.gdx); h->gdy = (float*)(w + L.gdy);
    h->kx_sum = w + L.kx_sum; h->kty_sum = w + L.kty_sum;
    h->part_blocks = L.part_blocks; h->rs_stride = L.rs_stride; h->rs_groups = L.rs_groups;
    for (int t = 0; t < 2; ++t) {
        Schedule& s = t == 0 ? h->sK : h->sKT;
        const Layout::LongRows& lr = L.long_rows[t];
        s.blk = (int64_t*)(w + L.sched[t]);
        s.rplo = (uint32_t*)(w + L.rplo[t]);
        s.lch = (int64_t*)(w + lr.lch); s.lrow = (int32_t*)(w + lr.lrow); s.lptr = (int32_t*)(w + lr.lptr); s.longpart = (void*)(w + lr.longpart);
        if (L.sharded) { s.ptab = (int32_t*)(w + L.ptab[t]); s.ptab_cap = L.ptab_cap[t]; }
    }
}

// The library's own stream and events (graph replay, early local-panel products).  Graph replay stays opt-in: on ROCm 7.2 / MI355X it
// measured 6-12 % SLOWER than direct launches on the small LPs it was meant for (neos3-shaped: 17.8k vs 20.2k it/s; 1M x 1M, 5
// nnz/row: 10.25k vs 10.86k it/s) -- the loop is bound by dependent-kernel latency on the device, not by host launch cost -- and
// makes no difference on large ones.
void open_side_stream(pdlp_handle h)
{
    h->side_ok = hipStreamCreateWithFlags(&h->gstream, hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming) == hipSuccess;
    if (!h->side_ok) {            // no side stream: no graph replay and no early local-panel products
        if (h->gstream) (void)hipStreamDestroy(h->gstream);
        h->gstream = nullptr;
        (void)hipGetLastError();
    }
}

int read_last_rowptr(const int64_t* rp, int64_t rows, int64_t* nnz, hipStream_t stream)
{
    // the arrays may just have been produced by kernels on the caller's stream (a non-blocking stream is not ordered
    // against the null stream's copy): read on that stream and wait
    int64_t v = 0;
    if (rows > 0) {
        HIP_TRY(hipMemcpyAsync(&v, rp + rows, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    *nnz = v;
    return PDLP_OK;
}

}  // namespace
