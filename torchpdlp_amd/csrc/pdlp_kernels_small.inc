// pdlp_kernels_small.inc -- scalar, vector and Ruiz kernels.
// Part of pdlp_hip.hip (included inside its anonymous namespace; not a translation unit of its own).
// ------------------------------------------------------------------------------------------------
// scalar kernels (one thread): the reference keeps eta/omega as 0-dim tensors of the working dtype
// ------------------------------------------------------------------------------------------------
template <typename T> __global__ void k_set_step(double* sc, double eta, double omega, double theta, double k)
{
    const T e = (T)eta, w = (T)omega, th = (T)theta;
    sc[S_ETA] = (double)e;
    sc[S_OMEGA] = (double)w;
    sc[S_THETA] = (double)th;
    sc[S_TAU] = (double)(T)(e / w);             // step.py:27 / :74
    sc[S_SIGMA] = (double)(T)(e * w);           // step.py:34 / :75
    sc[S_INV1PT] = (double)(T)((T)1 / ((T)1 + th));
    sc[S_K] = k;
}

// omega <- new primal weight (enhancements.py:77); tau, sigma follow from the eta currently on the device
template <typename T> __global__ void k_set_omega(double* sc, double omega)
{
    const T e = (T)sc[S_ETA], w = (T)omega;
    sc[S_OMEGA] = (double)w;
    sc[S_TAU] = (double)(T)(e / w);
    sc[S_SIGMA] = (double)(T)(e * w);
}

__global__ void k_reset_average(double* sc)
{
    sc[S_WPEND] = 0.0;
    sc[S_ETASUM] = 0.0;
}

// fixed step: eta_total += eta, k += 1, `iters` times (pdhg.py:76,109) in the working precision
template <typename T> __global__ void k_fixed_advance(double* sc, int iters)
{
    T s = (T)sc[S_ETASUM];
    const T e = (T)sc[S_ETA];
    for (int i = 0; i < iters; ++i) s = s + e;
    sc[S_ETASUM] = (double)s;
    sc[S_K] += (double)iters;
}

// adaptive rule, step.py:91-115 with quirk Q1 (one trial; a rejected step is kept), then
// pdhg.py:107-112: weight of the new iterate, eta_total, eta <- eta_hat.
// pw03 / pw06 = (k + 1)^-0.3 / ^-0.6 of the reference's 1-based k of this step (k1 = sc[S_K] + 1): passed in so that the
// one-workgroup kernel can evaluate the two double-precision pow() calls while its partial sums are still on their way
// QMAT (pdlp_objective_iterate: the linearised step of a sparse quadratic objective): red[3] holds the curvature dx'Q dx measured
// along the step, and the bound gains it -- eta_bar = (omega ||dx||^2 + ||dy||^2 / omega) / (2 |dy'K dx| + max(dx'Q dx, 0)), the
// descent-lemma condition ||dz||_M^2 >= dx'Q dx, exact for a quadratic (DESIGN.md 4.5.1).  Everything behind eta_bar is the LP's.
template <typename T, bool QMAT = false> __device__ void adaptive_rule(double* sc, const double* red, double k1, double pw03, double pw06)
{
    const T eta = (T)sc[S_ETA], omega = (T)sc[S_OMEGA];
    const T den = (T)2 * (T)red[2];                        // step.py:96
    T eta_bar, t1;
    [[maybe_unused]] T curv = (T)0, den_abs = (T)0;
    if constexpr (QMAT) {
        curv = (T)red[3];
        den_abs = (T)fabs((double)den) + (curv > (T)0 ? curv : (T)0);
    }
    if (QMAT ? den_abs != (T)0 : den != (T)0) {            // step.py:99-102
        const T nx = (T)sqrt(red[0]), ny = (T)sqrt(red[1]);
        const T num = omega * (nx * nx) + (ny * ny) / omega;
        if constexpr (QMAT) eta_bar = num / den_abs;
        else eta_bar = num / (T)fabs((double)den);
        t1 = (T)(1.0 - pw03) * eta_bar;
    } else {                                               // step.py:104-105
        eta_bar = (T)INFINITY;
        t1 = (T)INFINITY;
    }
    const T t2 = (T)(1.0 + pw06) * eta;                    // step.py:107
    const T eta_p = t1 < t2 ? t1 : t2;                     // step.py:108
    const bool accept = eta <= eta_bar;                    // step.py:110
    const T w = accept ? eta : eta_p;                      // first returned value (:111 / :115)
    sc[S_WPEND] = (double)w;
    sc[S_ETASUM_PREV] = sc[S_ETASUM];                      // (pdlp_adaptive_retry takes a rejected trial's weight out again, exactly)
    sc[S_ETASUM] = (double)(T)((T)sc[S_ETASUM] + w);       // pdhg.py:109
    sc[S_ETA] = (double)eta_p;                             // pdhg.py:112
    sc[S_TAU] = (double)(T)(eta_p / omega);
    sc[S_SIGMA] = (double)(T)(eta_p * omega);
    sc[S_K] = k1;
    sc[S_ACCEPT] = accept ? 1.0 : 0.0;
    sc[S_ETABAR] = (double)eta_bar;
    sc[S_DEN] = (double)den;
    if constexpr (QMAT) sc[S_CURV] = (double)curv;
}

// pdlp_adaptive_retry: the trial just taken is discarded (the intended loop of the adaptive step, enhancements/test_ass.py:322-363)
__global__ void k_retry_scalars(double* sc)
{
    sc[S_ETASUM] = sc[S_ETASUM_PREV];
    sc[S_WPEND] = 0.0;
    sc[S_K] -= 1.0;
}

template <typename T> __global__ void k_adaptive_update(double* sc, const double* red)
{
    const double k1 = sc[S_K] + 1.0;
    adaptive_rule<T>(sc, red, k1, pow(k1 + 1.0, -0.3), pow(k1 + 1.0, -0.6));
}

// single-rank fusion of pdlp_adaptive_reduce + pdlp_adaptive_update
// QMAT: a third array of partial sums, pq[b][0] of nq_blocks workgroups (the curvature, ObjGradStepEpi), added in the same fixed
// order into red[3], which nothing else uses while the rule runs
template <typename T, bool QMAT = false>
__device__ __forceinline__ void adaptive_reduce_body(const double* __restrict__ pa, int na_blocks, const double* __restrict__ pb, int nb_blocks,
                                                     double* __restrict__ red, double* __restrict__ sc, int update,
                                                     const double* __restrict__ pq = nullptr, int nq_blocks = 0)
{
    // This one-workgroup kernel sits between the two products of EVERY adaptive iteration: on small problems its latency is a
    // tenth of the iteration.  All partial sums of a thread are requested at once (unconditional loads on clamped block indices;
    // the additions keep the plain loop's order), and the three sums share one barrier.
    __shared__ double dred3[BLOCK / 64][QMAT ? 4 : 3];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    [[maybe_unused]] double s3 = 0.0;
    constexpr int U = 8;
    const double k1 = sc[S_K] + 1.0;                       // (wave uniform; thread 0 needs it)
    double pw03 = 0.0, pw06 = 0.0;
    int nmax = na_blocks > nb_blocks ? na_blocks : nb_blocks;
    if constexpr (QMAT) nmax = nq_blocks > nmax ? nq_blocks : nmax;
    const int la = na_blocks > 0 ? na_blocks - 1 : 0, lb = nb_blocks > 0 ? nb_blocks - 1 : 0;
    [[maybe_unused]] const int lq = nq_blocks > 0 ? nq_blocks - 1 : 0;
    for (int base = 0; base < nmax; base += BLOCK * U) {
        double va[U], vb[U], vc[U];
        [[maybe_unused]] double vq[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int b = base + u * BLOCK + (int)threadIdx.x;
            va[u] = pa[(size_t)(b < la ? b : la) * NACC];
            vb[u] = pb[(size_t)(b < lb ? b : lb) * NACC];
            vc[u] = pb[(size_t)(b < lb ? b : lb) * NACC + 1];
            if constexpr (QMAT) vq[u] = pq[(size_t)(b < lq ? b : lq) * NACC];      // (pq has room for one workgroup at least)
        }
        // the two pow() of the rule (hundreds of instructions in double precision) go here: behind the loads' issue, in front of
        // their first use
        __builtin_amdgcn_sched_barrier(0);
        if (base == 0 && update && threadIdx.x < 64) { pw03 = pow(k1 + 1.0, -0.3); pw06 = pow(k1 + 1.0, -0.6); }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int b = base + u * BLOCK + (int)threadIdx.x;
            s0 = b < na_blocks ? s0 + va[u] : s0;
            s1 = b < nb_blocks ? s1 + vb[u] : s1;
            s2 = b < nb_blocks ? s2 + vc[u] : s2;
            if constexpr (QMAT) s3 = b < nq_blocks ? s3 + vq[u] : s3;
        }
    }
    if (nmax <= 0 && update && threadIdx.x < 64) { pw03 = pow(k1 + 1.0, -0.3); pw06 = pow(k1 + 1.0, -0.6); }      // (no partial sums at all)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s0 += shfl_xor_t(s0, off);
        s1 += shfl_xor_t(s1, off);
        s2 += shfl_xor_t(s2, off);
        if constexpr (QMAT) s3 += shfl_xor_t(s3, off);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { dred3[w][0] = s0; dred3[w][1] = s1; dred3[w][2] = s2; }
    if constexpr (QMAT) { if (lane == 0) dred3[w][3] = s3; }
    __syncthreads();
    if (threadIdx.x == 0) {
        red[0] = dred3[0][0] + dred3[1][0] + dred3[2][0] + dred3[3][0];       // (block_sum's order)
        red[1] = dred3[0][1] + dred3[1][1] + dred3[2][1] + dred3[3][1];
        red[2] = dred3[0][2] + dred3[1][2] + dred3[2][2] + dred3[3][2];
        if constexpr (QMAT) red[3] = dred3[0][3] + dred3[1][3] + dred3[2][3] + dred3[3][3];
        if (update) adaptive_rule<T, QMAT>(sc, red, k1, pw03, pw06);
    }
}

template <typename T, bool QMAT = false>
__global__ __launch_bounds__(BLOCK) void k_adaptive_reduce_update(const double* __restrict__ pa, int na_blocks,
                                                                  const double* __restrict__ pb, int nb_blocks,
                                                                  double* __restrict__ red, double* __restrict__ sc, int update,
                                                                  const double* __restrict__ pq, int nq_blocks)
{
    adaptive_reduce_body<T, QMAT>(pa, na_blocks, pb, nb_blocks, red, sc, update, pq, nq_blocks);
}


// ---- direct exchange (pdlp_peer_*): flags and the step-size rule's sums in the ranks' mailboxes ---------------------------------
// The blocks themselves were stored into the peers' vectors by the half-step's epilogue (PeerOut); the kernel boundary in front of
// the signalling kernel has completed them.  Thread q tells peer q: "everything up to exchange `seq` of rank `me` is in your memory"
// -- and, for the exchange of y in an adaptive iteration, hands over this rank's three sums first (also into the own mailbox's slot).
struct PeerSignal {
    uint32_t* flag[MAX_PEER];      // slot `me` of each peer's mailbox
    double* sums[MAX_PEER];        // slot `me` of each peer's sums
    double* own_sums;              // slot `me` of the own mailbox
    uint32_t* own_flag;            // slot `me` of the own mailbox: the wait also waits for THIS rank's signal (it may come from a side stream)
    int n;
    uint32_t seq;
};
__device__ __forceinline__ void peer_signal_body(const PeerSignal& s, const double* red)
{
    const int q = (int)threadIdx.x;
    if (q == 0) {
        if (red)
            for (int c = 0; c < 3; ++c) __hip_atomic_store(s.own_sums + c, red[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(s.own_flag, s.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (q >= s.n) return;
    uint32_t* flag = s.flag[0];
    double* sums = s.sums[0];
#pragma unroll
    for (int i = 1; i < MAX_PEER; ++i)
        if (i == q) { flag = s.flag[i]; sums = s.sums[i]; }
    if (red)
        for (int c = 0; c < 3; ++c) __hip_atomic_store(sums + c, red[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(flag, s.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void k_peer_signal(PeerSignal s) { peer_signal_body(s, nullptr); }

// The push form of the direct exchange (PDLP_OPT_PEER_PUSH): the half-step's epilogue stores locally only, and this kernel -- on a side
// stream, beside the own-block panels of the next product -- copies the rank's block into every peer's vector (system-scope stores,
// written through); the signal follows it on that stream.  Link-bound: a modest grid leaves the chip to the product.
template <typename T> struct PeerPush { T* dst[MAX_PEER]; int n; };
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_peer_push(const T* __restrict__ src, PeerPush<T> d, int64_t len)
{
    // eight elements per thread in flight: a small grid (the few wave slots a chip-filling product leaves) must still feed a link
    constexpr int U = 8;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t i0 = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i0 < len; i0 += stride * U) {
        T v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = i0 + u * stride < len ? src[i0 + u * stride] : (T)0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (i0 + u * stride < len) {
#pragma unroll
                for (int q = 0; q < MAX_PEER; ++q)
                    if (q < d.n) __hip_atomic_store(d.dst[q] + i0 + u * stride, v[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// pdlp_adaptive_reduce and the signal of the y exchange in one launch: this rank's three sums, then flag and sums to every peer
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_adaptive_reduce_signal(const double* __restrict__ pa, int na_blocks, const double* __restrict__ pb,
                                                                  int nb_blocks, double* __restrict__ red, double* __restrict__ sc, PeerSignal s)
{
    adaptive_reduce_body<T>(pa, na_blocks, pb, nb_blocks, red, sc, 0);
    __syncthreads();                               // (thread 0 has written red)
    if (threadIdx.x < 64) peer_signal_body(s, (const double*)red);
}

// Thread q waits until rank q has signalled exchange `seq` (sequence numbers only grow; a peer can be one exchange ahead, never
// behind by more than the one being waited for).  A BOUNDED spin: after `limit` ticks of the 100 MHz clock the wave gives up, reports
// through *err (host memory: pdlp_peer_status) and ends -- the stream then runs on with incomplete vectors, which the host must not
// use; the grid always drains.
__device__ __forceinline__ void peer_wait_body(const uint32_t* box, int world, int me, uint32_t seq, long long limit, int* err)
{
    const int q = (int)threadIdx.x;
    if (q >= world) return;                       // (the own slot too: this rank's signal may be on its way on a side stream)
    const uint32_t* flag = box + (size_t)q * BOX_FLAG_STRIDE;
    const long long t0 = wall_clock64();
    while ((int32_t)(__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) - seq) < 0) {
        if (wall_clock64() - t0 > limit) {
            __hip_atomic_store(err, 1 + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
        __builtin_amdgcn_s_sleep(4);
    }
}
// Launched with PEER_WAIT_BLOCKS = 8 one-wave workgroups: consecutive workgroups go to consecutive XCDs, so every XCD runs one wave
// whose acquire (system scope: it invalidates what that XCD's L2 and L1 may hold of memory other agents write) follows the last
// flag -- whatever the next launch's own acquire covers, no XCD gathers a stale line of a vector the peers have just rewritten.
__global__ void k_peer_wait(const uint32_t* box, int world, int me, uint32_t seq, long long limit, int* err)
{
    peer_wait_body(box, world, me, seq, limit, err);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
}

// the wait for the y exchange of an adaptive iteration and pdlp_adaptive_update in one launch, the all-reduce done by hand: the
// ranks' sums, added in rank order (every rank gets the same bits)
template <typename T>
__global__ __launch_bounds__(64) void k_peer_wait_adaptive_update(const uint32_t* box, int world, int me, uint32_t seq, long long limit,
                                                                  int* err, double* sc, double* red)
{
    const double k1 = sc[S_K] + 1.0;
    double pw03 = 0.0, pw06 = 0.0;
    if (threadIdx.x == 0 && blockIdx.x == 0) { pw03 = pow(k1 + 1.0, -0.3); pw06 = pow(k1 + 1.0, -0.6); }      // (while the flags are on their way)
    peer_wait_body(box, world, me, seq, limit, err);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    __syncthreads();
    if (threadIdx.x != 0 || blockIdx.x != 0) return;         // (the other workgroups: their XCD's acquire only, see k_peer_wait)
    const double* box_sums = (const double*)((const char*)box + BOX_SUMS_AT);
    for (int c = 0; c < 3; ++c) {
        double s = 0.0;
        for (int q = 0; q < world; ++q) s += __hip_atomic_load(box_sums + (size_t)q * BOX_SUMS_STRIDE + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        red[c] = s;
    }
    adaptive_rule<T>(sc, red, k1, pw03, pw06);
}

// ------------------------------------------------------------------------------------------------
// vector kernels
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_flush(int64_t n, T* __restrict__ sum, const T* __restrict__ v, const double* sc, int widx)
{
    const T w = (T)sc[widx];           // S_WPEND (adaptive: the weight still pending) or S_ETA (fixed step: the K'y tail)
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) sum[i] += w * v[i];
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_average(int64_t n, T* __restrict__ avg, const T* __restrict__ sum, const double* sc)
{
    const T s = (T)sc[S_ETASUM];
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) avg[i] = sum[i] / s;
}

__global__ void k_clear_pending(double* sc) { sc[S_WPEND] = 0.0; }

// Sparse quadratic objective: the end of a KKT pass or report whose variable-side functor ran over g = c + Q x.  It left
// g'x = c'x + x'Qx in red[3]; with h = 1/2 x'Qx (red[xqx] holds x'Qx, the sum of ObjGradEpi) the contract of the six sums is
// red[3] = c'x + h and red[1] = its own term - h (include/pdlp_hip.h, pdlp_set_objective_matrix).
__global__ void k_obj_matrix_finish(double* red, int xqx)
{
    const double h = 0.5 * red[xqx];
    red[3] -= h;
    red[1] -= h;
}

// lam = project_lambda_box(g) (helpers.py:21-37) with the bound classes read off l, u.  project_lambda's arithmetic, written out as
// one expression: called here, the vectorised float32 loop of this kernel comes out with other selects.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_project_lambda(int64_t n, const T* __restrict__ g, const T* __restrict__ l,
                                                          const T* __restrict__ u, T* __restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const T lo = l[i], hi = u[i], gi = g[i];
        const bool ninf = isinf(lo) && lo < (T)0, pinf = isinf(hi) && hi > (T)0;
        out[i] = (ninf && pinf) ? (T)0 : (ninf ? (gi < (T)0 ? gi : (T)0) : (pinf ? (gi > (T)0 ? gi : (T)0) : gi));
    }
}

// out = a - b
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_sub(int64_t n, T* __restrict__ out, const T* __restrict__ a, const T* __restrict__ b)
{
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) out[i] = a[i] - b[i];
}

// out = a - b and partials[blk][0] = sum (a - b)^2 in double over the workgroup's elements: k_sub and k_sqdiff in one pass (a thread
// adds its elements in index order, then block_sum; no atomics, so the sums depend on n alone)
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_sub_sq(int64_t n, T* __restrict__ out, const T* __restrict__ a, const T* __restrict__ b,
                                                  double* __restrict__ partials)
{
    __shared__ double dred[4];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const T d = a[i] - b[i];
        out[i] = d;
        s += (double)d * (double)d;
    }
    s = block_sum(s, dred);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.x * NACC] = s;
}

// out = float(a - b): the float32 difference vector a delta-mode product gathers from
__global__ __launch_bounds__(BLOCK) void k_diff_f32(int64_t n, float* __restrict__ out, const double* __restrict__ a,
                                                    const double* __restrict__ b)
{
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) out[i] = (float)(a[i] - b[i]);
}

// partials[b][0] = sum (a-b)^2 (b may be null: sum a^2)
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_sqdiff(int64_t n, const T* __restrict__ a, const T* __restrict__ b,
                                                  double* __restrict__ partials)
{
    __shared__ double dred[4];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const T d = b ? a[i] - b[i] : a[i];
        s += (double)d * (double)d;
    }
    s = block_sum(s, dred);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.x * NACC] = s;
}

// v /= sqrt(red[idx])  (power iteration normalisation, helpers.py:50)
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_div_by_norm(int64_t n, T* __restrict__ v, const double* __restrict__ red, int idx)
{
    const T nb = (T)sqrt(red[idx]);
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) v[i] = v[i] / nb;
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_muldiv(int64_t n, T* __restrict__ a, const T* __restrict__ b, int op)
{
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK)
        a[i] = op ? a[i] / b[i] : a[i] * b[i];
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_max_dev_from_one(int64_t n, const T* __restrict__ v, double* __restrict__ out)
{
    __shared__ double dred[4];
    double mx = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const T d = (T)fabs((double)((T)1 - v[i]));
        mx = (double)d > mx ? (double)d : mx;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = shfl_xor_t(mx, off);
        mx = o > mx ? o : mx;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) dred[w] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) mx = dred[k] > mx ? dred[k] : mx;
        // non-negative doubles order like their bit patterns
        atomicMax((unsigned long long*)out, (unsigned long long)__double_as_longlong(mx));
    }
}

// ---- Ruiz building blocks: 8 lanes per row ------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_row_scale_factors(int64_t rows, const int64_t* __restrict__ rp,
                                                             const T* __restrict__ va, T eps, T* __restrict__ norm)
{
    const int64_t g = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 3;
    const int lt = threadIdx.x & 7;
    const int64_t stride = ((int64_t)gridDim.x * BLOCK) >> 3;
    for (int64_t i = g; i < ((rows + stride - 1) / stride) * stride; i += stride) {
        T mx = (T)0;
        if (i < rows)
            for (int64_t p = rp[i] + lt; p < rp[i + 1]; p += 8) {
                const T a = (T)fabs((double)va[p]);
                mx = a > mx ? a : mx;
            }
        for (int off = 4; off > 0; off >>= 1) {
            const T o = shfl_xor_t(mx, off);
            mx = o > mx ? o : mx;
        }
        if (i < rows && lt == 0) {
            const T r = (T)sqrt((double)mx);          // enhancements.py:49 / :54
            norm[i] = r < eps ? (T)1 : r;             // :50 / :55
        }
    }
}

// Pock-Chambolle factors (alpha = 1): norm[i] = sqrt(sum_p |va[p]|) over row i, 1 where the sum is 0 (an empty row, or stored zeros
// only).  k_row_scale_factors' lane layout; every lane adds its items p = rp[i] + lt, + 8, ... in double in that order, the eight
// partial sums meet in a 3-step butterfly (a + b == b + a: all eight lanes hold the same bits), one sqrt, one rounding to T.
// The order depends on the row alone, not on the grid.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_row_l1_factors(int64_t rows, const int64_t* __restrict__ rp, const T* __restrict__ va,
                                                          T* __restrict__ norm)
{
    const int64_t g = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 3;
    const int lt = threadIdx.x & 7;
    const int64_t stride = ((int64_t)gridDim.x * BLOCK) >> 3;
    for (int64_t i = g; i < ((rows + stride - 1) / stride) * stride; i += stride) {      // (uniform trip count: the shuffles need every lane)
        double s = 0.0;
        if (i < rows)
            for (int64_t p = rp[i] + lt; p < rp[i + 1]; p += 8) s += fabs((double)va[p]);
        for (int off = 4; off > 0; off >>= 1) s += shfl_xor_t(s, off);
        if (i < rows && lt == 0) norm[i] = s > 0.0 ? (T)sqrt(s) : (T)1;
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_div_rows(int64_t rows, const int64_t* __restrict__ rp, T* __restrict__ va,
                                                    const T* __restrict__ norm)
{
    const int64_t g = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 3;
    const int lt = threadIdx.x & 7;
    const int64_t stride = ((int64_t)gridDim.x * BLOCK) >> 3;
    for (int64_t i = g; i < rows; i += stride) {
        const T r = norm[i];
        for (int64_t p = rp[i] + lt; p < rp[i + 1]; p += 8) va[p] = va[p] / r;
    }
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_div_cols(int64_t nnz, const int32_t* __restrict__ ci, T* __restrict__ va,
                                                    const T* __restrict__ norm)
{
    for (int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * BLOCK)
        va[p] = va[p] / norm[ci[p]];
}

// ------------------------------------------------------------------------------------------------
// streaming-read probe: what this GPU reads with the tiled kernel's own access pattern (every workgroup its own contiguous
// slice, four 16-byte non-temporal loads in flight per thread) -- the measured ceiling next to the 8 TB/s spec in bench.py
// ------------------------------------------------------------------------------------------------
typedef unsigned int probe_u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(512) void k_probe_read(const probe_u32x4* __restrict__ a, size_t n16, unsigned* __restrict__ sink)
{
    const size_t per = n16 / gridDim.x;
    const probe_u32x4* p = a + (size_t)blockIdx.x * per;
    unsigned acc = 0;
    for (size_t i = threadIdx.x; i + 3 * 512 < per; i += 4 * 512) {
        probe_u32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(p + i + u * 512);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
    }
    if (acc == 0x12345678u) sink[0] = acc;            // (never true for the zero-filled buffer the caller passes; keeps the loads)
}

// pdlp_probe_gather: "8 bytes of item stream + one random 4-byte gather per item" in k_csr_fused's launch shape -- 256-thread
// workgroups striding over blocks of NNZ_CAP items, all item loads of a block in one round (unconditional), then all gathers.
// The ceiling of a CSR product whose gathers share no cache lines (5 non-zeros per row over 1M columns: one 128-byte line per gather).
__global__ __launch_bounds__(BLOCK) void k_probe_fill(uint32_t* __restrict__ idx, float* __restrict__ val, int64_t items, uint32_t entries)
{
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < items; i += (int64_t)gridDim.x * BLOCK) {
        uint64_t z = (uint64_t)i * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;          // splitmix64: uniform columns
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        idx[i] = (uint32_t)(z % entries);
        val[i] = 1.0f;
    }
}

__global__ __launch_bounds__(BLOCK) void k_probe_gather(const uint32_t* __restrict__ idx, const float* __restrict__ val,
                                                        const float* __restrict__ table, int64_t items, float* __restrict__ sink)
{
    constexpr int UNR = NNZ_CAP / BLOCK;
    const int64_t nblk = items / NNZ_CAP;
    float acc = 0.f;
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
        const int64_t a = b * NNZ_CAP + threadIdx.x;
        float v[UNR];
        uint32_t c[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) { v[u] = val[a + u * BLOCK]; c[u] = idx[a + u * BLOCK]; }
#pragma unroll
        for (int u = 0; u < UNR; ++u) v[u] *= table[c[u]];
#pragma unroll
        for (int u = 0; u < UNR; ++u) acc += v[u];
    }
    if (acc == 123.456f) sink[0] = acc;               // (the table is zero: never true; keeps the loads)
}
