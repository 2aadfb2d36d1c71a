// ba_k5_panel.hpp -- K5 on the matrix cores for <= 10 free keyframes (RSVIO_K5=mfma, the
// default): MfDims, the dense map, the partial-system combines, mf_pivot / mf_factor / mf_update /
// mf_panel, camera_solve_mfma_body and its two kernels (ba_camera_solve_mfma, _mfma_p2p).
// Part of ba.hip's translation unit: included by ba.hip inside its file-local namespace, after
// the types, the P2P helpers and the shared K5 helpers (k5_finish, k5_result, rl64) it uses.
#pragma once

// ---------------------------------------------------------------------------------------
// K5 on the matrix cores (n <= 60; RSVIO_K5=mfma): blocked right-looking
// LDL^T of the camera system with 16-column panels.  The system (padded to NPP = 16 ceil(n/16)
// with identity rows / columns, which couple to nothing) sits column-major in LDS.  Per panel:
//   * wave 0 (lane = row) factors the panel's columns in registers -- per pivot K the 1/d_K
//     chain (v_rcp_f64 + the folded Newton step), l = u / d_K, the in-panel updates from
//     readlanes of the unscaled column, and b_i -= l_iK b_K (so b ends as L^-1 b) -- and writes
//     L into the panel's columns of M, U = D L into Up;
//   * every wave then updates its share of the trailing lower tiles (I, J > panel) with
//     v_mfma_f64_16x16x4_f64: C_IJ += (-U_I) L_J^T over the panel's 16 columns (4 MFMAs per
//     tile, accumulator in registers, C loaded from / stored to M).
// The serial chain is the pivots inside the panels; the O(n^3) trailing work runs on the matrix
// cores, off wave 0's chain.  z = D^-1 L^-1 b, then L^T x = z by wave 0 (readlanes, as pipe4).
// Tolerance parity like pipe4 (same pivots; the trailing sums reassociated by the MFMA).
// ---------------------------------------------------------------------------------------
typedef double mf_dbl4 __attribute__((ext_vector_type(4)));
constexpr int kMfLd = 65;  // f64 leading dimension of the LDS matrices (odd: column reads spread banks)
constexpr int kMfPanel = 8;  // panel width: 8 pivots of in-panel VALU work between matrix-core updates

// The augmented system [[S, .], [b^T, .]] padded to NPP = 16 NT >= NP + 1 rows: row NP is b, so
// eliminating the augmented matrix turns row NP into z^T = (D^-1 L^-1 b)^T on the fly (one more
// row of every panel).  Rows past NP are never initialised: elimination is row-local (a row's
// update uses its own multiplier and the pivot rows' values), so they cannot leak into the
// result; the same holds for the upper halves of the diagonal tiles.
template <int NF>
struct MfDims {
    static constexpr int NP = 6 * NF;
    static constexpr int NT = NP / 16 + 1;
    static constexpr int NPP = 16 * NT;
    static constexpr int NH = (NP + kMfPanel - 1) / kMfPanel;  // panels
};

// Per packed-system entry (sys layout: n_pb x 36 S | 6 n_free b | 6 n_free g_c) its destination
// in K5's LDS: >= 0 a column-major position of M (bit 30: + lambda after the sum), -1 none (the
// upper half of a diagonal block), -2 - i the i-th g_c.  Built on the host per problem.
constexpr int kMfMapLambda = 1 << 30;
inline void mf_dense_map(int nf, int n_pb, const int* pb_fa, const int* pb_fb, int* map, int np_target = 0,
                         int ld = kMfLd) {
    const int np = np_target > 0 ? np_target : 6 * nf;  // the b row (the template's NP)
    for (int pb = 0; pb < n_pb; ++pb)
        for (int k = 0; k < 36; ++k) {
            const int ra = k / 6, ca = k % 6, fa = pb_fa[pb], fb = pb_fb[pb];
            int v;
            if (fa == fb)
                v = ra >= ca ? ((6 * fa + ca) * ld + 6 * fa + ra) | (ra == ca ? kMfMapLambda : 0) : -1;
            else
                v = (6 * fa + ra) * ld + 6 * fb + ca;  // S[6fa+ra][6fb+ca] -> its lower mirror
            map[36 * pb + k] = v;
        }
    for (int i = 0; i < 6 * nf; ++i) map[36 * n_pb + i] = i * ld + np;  // b_i -> row NP, column i
    for (int i = 0; i < 6 * nf; ++i) map[36 * n_pb + 6 * nf + i] = -2 - i;
}

// combine_system with the sums scattered straight into M (and g_c into gsh) by the map
// The partial systems' loads are issued before the LM state's (whose done flag decides whether
// anything is stored and whose lambda joins the diagonal), so the state's round trip overlaps
// theirs.  Returns the state's done flag (nothing stored then).
template <int NF>
__device__ bool combine_mapped(const Geometry& G, const Prob& Pr, const Work& Wk, double* M, double* gsh,
                               const LmState* st, int* fail) {
    constexpr int NE = (NF * (NF + 1) / 2) * 36 + 12 * NF;  // the template's (upper bound)
    constexpr int T = kK5Threads, kE = (NE + T - 1) / T;
    const size_t L = sys_len(G);
    const int ne = G.n_pb * 36 + 12 * G.n_free;  // this window's entries (batched: may be fewer)
    const int tid = threadIdx.x;
    double v[kE][kGrp];
    int dst[kE];
#pragma unroll
    for (int i = 0; i < kE; ++i) {  // (branch-free: clamped loads; an entry past ne is never stored)
        const int e = tid + T * i, ec = min(e, ne - 1);
        const int d = Pr.dmap[ec];
        dst[i] = e < ne ? d : -1;
#pragma unroll
        for (int x = 0; x < kGrp; ++x) v[i][x] = Wk.cpart[(size_t)x * L + ec];
    }
    // then the K4 wave partials (initial cost) and the singular flag, behind them (branch-free:
    // clamped loads, the ones past the last wave dropped at the sum -- a zeroing select here made
    // the compiler wait for these loads before issuing the partial systems')
    double pa[16];
    int sing = 0;
    if (tid < 64) {
        const int wl = max(G.n_wave - 1, 0);
#pragma unroll
        for (int k = 0; k < 16; ++k) pa[k] = Wk.partA[min(tid + 64 * k, wl) * kPartA];
        sing = *Wk.singular;
    }
    const int done = st->done;
    const double lambda = st->lambda;
    // keep the compiler from sinking the partial systems' loads under the done branch
#pragma unroll
    for (int i = 0; i < kE; ++i)
#pragma unroll
        for (int x = 0; x < kGrp; ++x) __asm__ volatile("" ::"v"(v[i][x]));
    if (done) return true;
#pragma unroll
    for (int i = 0; i < kE; ++i) {
        double a = v[i][0];
#pragma unroll
        for (int x = 1; x < kGrp; ++x) a += v[i][x];
        const int d = dst[i];
        if (d >= 0) {
            if (d & kMfMapLambda) a += lambda;
            M[d & (kMfMapLambda - 1)] = a;
        } else if (d <= -2) {
            gsh[-2 - d] = a;
        }
    }
    if (tid < 64) {
        double c = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) c += tid + 64 * k < G.n_wave ? pa[k] : 0.0;
        for (int w = tid + 64 * 16; w < G.n_wave; w += 64) c += Wk.partA[w * kPartA];
        c = wave_sum_det(c);
        if (tid == 0) {
            Wk.sys[G.n_pb * 36 + 12 * G.n_free] = c;  // the decision of iteration 0 reads the initial cost here
            *fail = sing;
        }
    }
    return false;
}

// combine_p2p's exchange in flag-in-word form (RSVIO_P2P_LL=1, A/B): every entry (and the three
// scalars: initial cost, singular flag, wave count) goes to every rank as two tagged 8-byte words
// -- no fence, no flags -- and the reader polls the words themselves, every rank's words of its
// entries in flight together (ranks in two groups of 4), re-reading until all carry this
// exchange's tag.  Same sums in the same rank order as the flag protocol: the same bits.
template <int NF>
__device__ bool combine_p2p_ll(const Geometry& G, const Work& Wk, double* M, double* gsh, int* fail, const P2P& P,
                               unsigned long long* xgen, int* err,
                               const double (&v)[((NF * (NF + 1) / 2) * 36 + 12 * NF + kK5Threads - 1) / kK5Threads][kGrp],
                               const int (&dst)[((NF * (NF + 1) / 2) * 36 + 12 * NF + kK5Threads - 1) / kK5Threads],
                               const double (&pa)[16], int sing, double lambda, unsigned long long gen) {
    constexpr int NE = (NF * (NF + 1) / 2) * 36 + 12 * NF;
    constexpr int T = kK5Threads, kE = (NE + T - 1) / T;
    const int ne = G.n_pb * 36 + 12 * G.n_free;
    const int tid = threadIdx.x, nr = P.nranks, me = P.rank, par = (int)(gen & 1);
    const unsigned g32 = (unsigned)gen;
#pragma unroll
    for (int i = 0; i < kE; ++i) {
        const int e = tid + T * i;
        if (e >= ne) break;
        double a = v[i][0];
#pragma unroll
        for (int x = 1; x < kGrp; ++x) a += v[i][x];
        if (me == 0 && dst[i] >= 0 && (dst[i] & kMfMapLambda)) a += lambda;
        for (int r = 0; r < nr; ++r) ll_put(p2p_llsys(P.peer[r], par, me) + 2 * (size_t)e, a, g32);
    }
    double c = 0.0;
    if (tid < 64) {
#pragma unroll
        for (int k = 0; k < 16; ++k) c += tid + 64 * k < G.n_wave ? pa[k] : 0.0;
        for (int w = tid + 64 * 16; w < G.n_wave; w += 64) c += Wk.partA[w * kPartA];
        c = wave_sum_det(c);
    }
    // the scalars go last, once every thread's entry stores have completed (vmcnt(0), then the
    // barrier), so a reader that sees a rank's scalars finds its entries there too: the readers
    // poll the 6 scalar words of each rank and read the entries once (still tag-checked), instead
    // of every thread re-reading all its entries' words of every rank until they arrive -- traffic
    // that, with four ranks on one GPU, starved the last rank's own progress until the spin bound
    __builtin_amdgcn_s_waitcnt(kWaitStores);
    __syncthreads();
    if (tid < nr) {  // lane r pushes the scalars to rank r
        unsigned long long* d = p2p_llsys(P.peer[tid], par, me) + 2 * (size_t)ne;
        ll_put(d, c, g32);
        ll_put(d + 2, sing ? 1.0 : 0.0, g32);
        ll_put(d + 4, (double)G.n_wave, g32);
    }
    const unsigned long long* mine = p2p_llsys(P.peer[me], par, 0);
    // scalars: lane r of wave 0 reads rank r's three (the sums in rank order by lane 0, below)
    __shared__ double sc[kP2PMax][3];
    if (tid < nr) {
        const unsigned long long* a = mine + (size_t)tid * 2 * kP2PMsg + 2 * (size_t)ne;
        unsigned long long ws[6];
        long long spins = 0;
        for (;;) {
#pragma unroll
            for (int k = 0; k < 6; ++k) ws[k] = __hip_atomic_load(a + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            bool ok = true;
#pragma unroll
            for (int k = 0; k < 6; ++k) ok &= (unsigned)(ws[k] >> 32) == g32;
            if (ok) break;
            if (++spins > (1ll << 25)) {
                atomicExch(err, 1);
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
            sc[tid][k] = __longlong_as_double((long long)((ws[2 * k] & 0xffffffffull) | (ws[2 * k + 1] << 32)));
    }
    __syncthreads();
    // entries: every rank's two words of this thread's entries, ranks in groups of 2 or 4
    double acc[kE];
#pragma unroll
    for (int i = 0; i < kE; ++i) acc[i] = 0.0;
    const bool late = nr <= 2 ? ll_group_sums<kE, 2>(mine, nr, ne, tid, T, g32, acc)
                              : ll_group_sums<kE, 4>(mine, nr, ne, tid, T, g32, acc);
    if (late) atomicExch(err, 1);
#pragma unroll
    for (int i = 0; i < kE; ++i) {
        const int e = tid + T * i;
        if (e >= ne) break;
        const int d = dst[i];
        if (d >= 0)
            M[d & (kMfMapLambda - 1)] = acc[i];
        else if (d <= -2)
            gsh[-2 - d] = acc[i];
    }
    if (tid == 0) {
        double cs = 0.0, f = 0.0;
        for (int r = 0; r < nr; ++r) {
            cs += sc[r][0];
            f += sc[r][1];
        }
        Wk.sys[ne] = cs;  // the decision of iteration 0 reads the (all-reduced) initial cost here
        *fail = f != 0.0;
        *xgen = gen;
    }
    if (tid < nr && P.xnw) P.xnw[tid] = (int)sc[tid][2];
    return false;
}

// combine_mapped for the landmark-sharded path over the P2P exchange (X1 folded into K5): this
// rank's reduced system is summed from its partials as combine_mapped does (+ lambda on rank 0,
// after the sum, as K4d), each entry pushed from its register into slot [parity][rank] of every
// peer's exchange buffer together with the rank's initial cost and singular flag; after the
// system-scope flags of every rank have arrived, each thread sums its entries over the slots in
// RANK ORDER (identical bits on every rank, and the same bits as X1's exchange into sys followed
// by K5's read of sys) and scatters them into M / gsh by the map.  Returns the state's done flag:
// every rank takes the same decision, so either all exchange or none does.  LL: the flag-in-word
// form (combine_p2p_ll) -- a kernel of its own, so that its polling loops' registers do not
// inflate the flag protocol's (one kernel holding both took 399 VGPRs, AGPR copies on the
// prologue's path, +1.3 us per K5 at one rank against the unsharded combine)
template <int NF, bool LL>
__device__ bool combine_p2p(const Geometry& G, const Prob& Pr, const Work& Wk, double* M, double* gsh,
                            const LmState* st, int* fail, const P2P& P, unsigned long long* xgen, int* err) {
    constexpr int NE = (NF * (NF + 1) / 2) * 36 + 12 * NF;
    constexpr int T = kK5Threads, kE = (NE + T - 1) / T;
    const size_t L = sys_len(G);
    const int ne = G.n_pb * 36 + 12 * G.n_free;
    const int tid = threadIdx.x, nr = P.nranks, me = P.rank;
    // the exchange's generation: loaded by every thread (one address), waited for at its first
    // use after the partial systems' loads are in flight -- not an LDS broadcast by one thread,
    // whose store made wave 0 wait a whole round trip (with the pose loads ahead of it) before
    // issuing its share of those loads, and cost a barrier
    const unsigned long long gen0 = *xgen;
    double v[kE][kGrp];
    int dst[kE];
#pragma unroll
    for (int i = 0; i < kE; ++i) {  // (branch-free: clamped loads; an entry past ne is never stored)
        const int e = tid + T * i, ec = min(e, ne - 1);
        const int d = Pr.dmap[ec];
        dst[i] = e < ne ? d : -1;
#pragma unroll
        for (int x = 0; x < kGrp; ++x) v[i][x] = Wk.cpart[(size_t)x * L + ec];
    }
    // then the K4 wave partials (initial cost) and the singular flag, behind them (branch-free:
    // clamped loads, the ones past the last wave dropped at the sum -- a zeroing select here made
    // the compiler wait for these loads before issuing the partial systems')
    double pa[16];
    int sing = 0;
    if (tid < 64) {
        const int wl = max(G.n_wave - 1, 0);
#pragma unroll
        for (int k = 0; k < 16; ++k) pa[k] = Wk.partA[min(tid + 64 * k, wl) * kPartA];
        sing = *Wk.singular;
    }
    const int done = st->done;
    const double lambda = st->lambda;
#pragma unroll
    for (int i = 0; i < kE; ++i)
#pragma unroll
        for (int x = 0; x < kGrp; ++x) __asm__ volatile("" ::"v"(v[i][x]));
    if (done) return true;
    const unsigned long long gen = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)gen0) +
                                   ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(gen0 >> 32)) << 32) + 1;
    const int par = (int)(gen & 1);
    if constexpr (LL) return combine_p2p_ll<NF>(G, Wk, M, gsh, fail, P, xgen, err, v, dst, pa, sing, lambda, gen);
    // this rank's entries stay in registers (own): only the peers' slots are written, flagged,
    // waited for and read back (round 5; the own slot's uncached write, flag and re-read were the
    // exchange's whole cost at one rank)
    double own[kE];
#pragma unroll
    for (int i = 0; i < kE; ++i) {
        const int e = tid + T * i;
        double a = v[i][0];
#pragma unroll
        for (int x = 1; x < kGrp; ++x) a += v[i][x];
        if (me == 0 && dst[i] >= 0 && (dst[i] & kMfMapLambda)) a += lambda;
        own[i] = a;
        if (e < ne)
            for (int r = 0; r < nr; ++r)
                if (r != me) p2p_slot(P.peer[r], par, me)[e] = a;
    }
    __shared__ double osc[2];  // this rank's initial cost and singular flag
    if (tid < 64) {
        double c = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) c += tid + 64 * k < G.n_wave ? pa[k] : 0.0;
        for (int w = tid + 64 * 16; w < G.n_wave; w += 64) c += Wk.partA[w * kPartA];
        c = wave_sum_det(c);
        if (tid == 0) {
            osc[0] = c;
            osc[1] = sing ? 1.0 : 0.0;
        }
        if (tid < nr && tid != me) {  // lane r pushes the scalars to rank r
            double* d = p2p_slot(P.peer[tid], par, me);
            d[ne] = c;
            d[ne + 1] = sing ? 1.0 : 0.0;
            d[ne + 2] = (double)G.n_wave;  // (per rank, not summed: the folded trial exchange's bound)
        }
    }
    if (nr > 1) __threadfence_system();
    __syncthreads();
    if (tid < nr && tid != me)
        __hip_atomic_store(p2p_flags(P.peer[tid]) + par * kP2PMax + me, gen, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    if (tid < nr && tid != me) {
        const unsigned long long* f = p2p_flags(P.peer[me]) + par * kP2PMax + tid;
        long long spins = 0;
        while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < gen) {
            __builtin_amdgcn_s_sleep(2);
            if (++spins > (1ll << 25)) {  // a peer never arrived: report, do not hang
                atomicExch(err, 1);
                break;
            }
        }
        // relaxed polls (no L2 invalidate per poll), one acquire once the flag is seen
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    }
    __syncthreads();
    const double* mine = p2p_slot(P.peer[me], par, 0);
    // this thread's values from a group of ranks in flight together (own from registers, peers'
    // from their slots), groups in rank order: one round trip per group of 2 (two ranks), 4 (three
    // or four) or 8 ranks, then the rank-ordered sums
    double sums[kE];
#pragma unroll
    for (int i = 0; i < kE; ++i) sums[i] = 0.0;
    if (nr <= 2)
        p2p_group_sums_own<kE, 2>(mine, nr, me, ne, tid, T, own, sums);
    else if (nr <= 4)
        p2p_group_sums_own<kE, 4>(mine, nr, me, ne, tid, T, own, sums);
    else  // 5..8 ranks: every peer's slot in flight together -- one round trip, not two groups of 4
        p2p_group_sums_own<kE, 8>(mine, nr, me, ne, tid, T, own, sums);
#pragma unroll
    for (int i = 0; i < kE; ++i) {
        const int e = tid + T * i;
        if (e >= ne) break;
        const double a = sums[i];
        const int d = dst[i];
        if (d >= 0)
            M[d & (kMfMapLambda - 1)] = a;
        else if (d <= -2)
            gsh[-2 - d] = a;
    }
    if (tid == 0) {
        // every peer's two scalars in flight together (unrolled over the rank bound), then the
        // rank-ordered sums with this rank's own values substituted
        double cv[kP2PMax], fv[kP2PMax];
#pragma unroll
        for (int r = 0; r < kP2PMax; ++r) {
            const bool peer = r < nr && r != me;
            cv[r] = peer ? __hip_atomic_load(mine + (size_t)r * kP2PMsg + ne, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                         : osc[0];
            fv[r] = peer ? __hip_atomic_load(mine + (size_t)r * kP2PMsg + ne + 1, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_SYSTEM)
                         : osc[1];
        }
        double c = 0.0, f = 0.0;
#pragma unroll
        for (int r = 0; r < kP2PMax; ++r)
            if (r < nr) {
                c += cv[r];
                f += fv[r];
            }
        Wk.sys[ne] = c;  // the decision of iteration 0 reads the (all-reduced) initial cost here
        *fail = f != 0.0;
        *xgen = gen;
    }
    if (tid < nr && P.xnw)
        P.xnw[tid] = tid == me ? G.n_wave
                               : (int)__hip_atomic_load(mine + (size_t)tid * kP2PMsg + ne + 2, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_SYSTEM);
    return false;
}

// pivot J of panel H (width PW) by wave 0: inv = 1 / d_K ready.  Column J+1 (the next pivot's)
// and column J+2 are updated from readlanes of the unscaled column u; columns >= J+3 from values
// of u read this step and consumed one step later (uq, with the pivot's l as lp) -- by readlane
// since round 6 (LDS broadcasts before: their wait sat between two pivots' chains).
template <int H, int J, int PW, bool KD = false>
__device__ __forceinline__ void mf_pivot(double (&a)[kMfPanel], double (&uq)[kMfPanel], double lp, double inv,
                                         double* Lf, double* Up, int lane, bool& bad, double* Dv = nullptr) {
    constexpr int K = kMfPanel * H + J;
    const double u = a[J];
    if constexpr (KD)  // 1 / d_K kept (the covariance inverts the factor)
        if (lane == 0) Dv[K] = inv;
    double inv_next = 1.0;
    double uk1 = 0.0;
    if constexpr (J + 1 < PW) {
        // the next pivot on the shortest chain: d_{K+1} = a_{K+1,K+1} - u_{K+1,K}^2 / d_K, with
        // u_{K+1,K} and a_{K+1,K+1} read before 1/d_K is known -- inv -> fma -> rcp (+ Newton),
        // uniform on every lane, no readlane on the chain
        uk1 = rl64(u, K + 1);
        const double piv = fma(-(uk1 * uk1), inv, rl64(a[J + 1], K + 1));
        bad |= !(piv > 0.0) || !isfinite(piv);
        // the hardware reciprocal issued here, before the barrier (round 6): left to the
        // compiler, IR code sinking moved it past this pivot's other updates, so ~12 issue slots
        // sat between the pivot and its reciprocal on the 1/d chain; the Newton steps follow where
        // the next pivot needs them (rcp_f64's operations, the same bits).  Measured neutral
        // (0.0302-0.0304 ms per LM iteration either way, profiles/r06i_rcp_ab.txt): the chain's
        // issue slots, not this placement, bound it
        double y0 = __builtin_amdgcn_rcp(piv);
        __asm__ volatile("" : "+v"(y0));
        const double e = fma(-piv, y0, 1.0);
        inv_next = fma(y0, fma(e, e, e), y0);
    }
    const double l = u * inv;
    if constexpr (J + 1 < PW) a[J + 1] = fma(-l, uk1, a[J + 1]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (J > 0)
#pragma unroll
        for (int jj = J + 2; jj < PW; ++jj) a[jj] = fma(-lp, uq[jj], a[jj]);
    if constexpr (J + 2 < PW) a[J + 2] = fma(-l, rl64(u, K + 2), a[J + 2]);
    Lf[K * kMfLd + lane] = l;  // column K of L (rows > K; row NP: z_K); the upper part is never read
    Up[J * kMfLd + lane] = u;  // column J of the panel's U = D L
    // round 6: the later columns' multipliers by readlane too -- no LDS read and no wait on it
    // between this pivot's chain and the next (0.0305 -> 0.0302 ms per LM iteration, 3 of 3 A/B
    // pairs, profiles/r06h_rlq_ab.txt) than by LDS broadcasts of Up's column (round 3-5)
#pragma unroll
    for (int jj = J + 3; jj < PW; ++jj) uq[jj] = rl64(u, kMfPanel * H + jj);
    if constexpr (J + 1 < PW) mf_pivot<H, J + 1, PW, KD>(a, uq, l, inv_next, Lf, Up, lane, bad, Dv);
}

// Panel H (columns 8H .. 8H + PW - 1) factored by wave 0 from M into Lf and its U buffer Uh.
template <int NF, int H, bool KD = false>
__device__ __forceinline__ void mf_factor(const double* M, double* Lf, double* Uh, int lane, bool& bad,
                                          double* Dv = nullptr) {
    constexpr int NP = MfDims<NF>::NP;
    constexpr int C0 = kMfPanel * H;
    constexpr int PW = (NP - C0) < kMfPanel ? (NP - C0) : kMfPanel;
    double a[kMfPanel], uq[kMfPanel];
#pragma unroll
    for (int jj = 0; jj < kMfPanel; ++jj) {
        a[jj] = jj < PW ? M[(C0 + jj) * kMfLd + lane] : 0.0;
        uq[jj] = 0.0;
    }
    const double piv = rl64(a[0], C0);
    bad |= !(piv > 0.0) || !isfinite(piv);
    mf_pivot<H, 0, PW, KD>(a, uq, 0.0, rcp_f64(piv), Lf, Uh, lane, bad, Dv);
}

// The trailing update of panel H on the matrix cores: lower tiles (I, J), I >= J, of tile columns
// J0 <= J < J1, C_IJ += (-U_I) L_J^T over the panel's 8 columns (2 MFMAs per tile), tile t of the
// flattened list taken by wave `wid` of `nw`.  A tile holding factored columns gets garbage there
// (their L lives in Lf).
template <int NF, int H>
__device__ __forceinline__ void mf_update(double* M, const double* Lf, const double* Uh, int lane, int wid, int nw,
                                          int J0, int J1) {
    constexpr int NT = MfDims<NF>::NT;
    constexpr int C0 = kMfPanel * H;
    const int i16 = lane & 15, k4 = lane >> 4;
    int ntile = 0;
    for (int J = J0; J < J1; ++J) ntile += NT - J;
    for (int t = wid; t < ntile; t += nw) {
        int TJ = J0, rem = t;
        while (rem >= NT - TJ) {
            rem -= NT - TJ;
            ++TJ;
        }
        const int TI = TJ + rem;
        double av[2], bv[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int kk = 4 * m + k4;
            av[m] = -Uh[kk * kMfLd + 16 * TI + i16];
            bv[m] = Lf[(C0 + kk) * kMfLd + 16 * TJ + i16];
        }
        mf_dbl4 c;
#pragma unroll
        for (int r = 0; r < 4; ++r) c[r] = M[(16 * TJ + i16) * kMfLd + 16 * TI + k4 + 4 * r];
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0], bv[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1], bv[1], c, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) M[(16 * TJ + i16) * kMfLd + 16 * TI + k4 + 4 * r] = c[r];
    }
}

// Panel H is factored (Lf, Up[H & 1]) and visible to every wave.  Look-ahead: wave 0 updates the
// tile column T0 that holds panel H + 1's columns and factors panel H + 1 straight away (into the
// other U buffer), while waves 1-3 update the tile columns past T0 -- disjoint columns of M, so
// the next pivot chain starts without waiting for the rest of the trailing update.
template <int NF, int H, bool KD = false>
__device__ __forceinline__ void mf_panel(double* M, double* Lf, double* Up, int tid, bool& bad, double* Dv = nullptr) {
    constexpr int NT = MfDims<NF>::NT, NH = MfDims<NF>::NH;
    constexpr int C0 = kMfPanel * H;
    const int lane = tid & 63, wave = tid >> 6;
    if constexpr (H == 0) STAMP(9); else if constexpr (H == 2) STAMP(15); else if constexpr (H == 4) STAMP(30);
    if constexpr (H + 1 == NH) STAMP(7);
    if constexpr (H + 1 < NH) {
        constexpr int T0 = (C0 + kMfPanel) / 16;  // the tile column of panel H + 1
        double* Uh = Up + (H & 1) * kMfPanel * kMfLd;
        if (wave == 0) {
            mf_update<NF, H>(M, Lf, Uh, lane, 0, 1, T0, T0 + 1);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the column's updates before its reads
            __builtin_amdgcn_wave_barrier();
            mf_factor<NF, H + 1, KD>(M, Lf, Up + ((H + 1) & 1) * kMfPanel * kMfLd, lane, bad, Dv);
        } else {
            mf_update<NF, H>(M, Lf, Uh, lane, wave - 1, kK5Threads / 64 - 1, T0 + 1, NT);
        }
        __syncthreads();
        if constexpr (H == 0) STAMP(13); else if constexpr (H == 2) STAMP(19); else if constexpr (H == 4) STAMP(31);
        mf_panel<NF, H + 1, KD>(M, Lf, Up, tid, bad, Dv);
    }
}

template <int NF, bool LL = false>
__device__ void camera_solve_mfma_body(const Geometry& G, const Prob& Pr, const Work& Wk, int combine,
                                       const P2P* P = nullptr, unsigned long long* xgen = nullptr, int* err = nullptr) {
    static_assert(NF >= 1 && NF <= 10, "one row per lane: n <= 60");
    constexpr int NP = MfDims<NF>::NP, NPP = MfDims<NF>::NPP;
    __shared__ __attribute__((aligned(16))) double M[NPP * kMfLd];
    __shared__ __attribute__((aligned(16))) double Lf[NPP * kMfLd];
    __shared__ __attribute__((aligned(16))) double Up[2 * kMfPanel * kMfLd];  // U of panels H & 1
    __shared__ double gsh[NP];
    __shared__ int fail;
    RTSTAMP(4);
    LmState* st = Wk.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nF = G.n_free, n = 6 * nF;
    const int SC0 = G.n_pb * 36 + 12 * nF;
    // both pose buffers (the state's cur picks one), loaded with the partial systems, before the
    // state itself
    double p7b[2][7];
    int fidx = -1;
    if (wave == 0 && lane < G.n_kf) {
        fidx = Pr.free_idx[lane];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 7; ++i) p7b[b][i] = Wk.pose[b][7 * lane + i];
    } else {
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 7; ++i) p7b[b][i] = i == 3 ? 1.0 : 0.0;
    }
    STAMP(0);
    if (combine == 2) {  // sharded over P2P: this rank's system exchanged in the prologue (X1 folded in)
        if (combine_p2p<NF, LL>(G, Pr, Wk, M, gsh, st, &fail, *P, xgen, err)) return;
    } else if (combine) {
        if (combine_mapped<NF>(G, Pr, Wk, M, gsh, st, &fail)) return;
    } else {  // sharded: the all-reduced system (+ lambda on the owner rank) from sys, by the map
        if (st->done) return;
        const double* sys = Wk.sys;
        const int ne = G.n_pb * 36 + 12 * nF;
        for (int e = tid; e < ne; e += kK5Threads) {
            const int d = Pr.dmap[e];
            if (d >= 0)
                M[d & (kMfMapLambda - 1)] = sys[e];
            else if (d <= -2)
                gsh[-2 - d] = sys[e];
        }
        if (tid == 0) fail = sys[SC0 + 1] != 0.0;
    }
    const int cur = st->cur;
    double p7[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) p7[i] = cur ? p7b[1][i] : p7b[0][i];
    if (n < NP) {
        // a window with fewer free keyframes than the template (batched mode): its rows and
        // columns [n, NP) are identity padding, and the b row is zero there
        for (int e = tid; e < NP * (NP + 1); e += kK5Threads) {
            const int c = e / (NP + 1), r = e - c * (NP + 1);
            if (r >= c && ((r >= n && r < NP) || (c >= n && c < NP))) M[c * kMfLd + r] = r == c ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    STAMP(1);
    // the singular flag of this iteration's K4c is already in fail (combine_mapped / combine_p2p
    // load it with the partial systems; the sys path's K4d / X1 carried it and cleared it): only
    // its reset for the next iteration here (re-reading it cost a round trip on the chain)
    if (tid == 0) *Wk.singular = 0;
    const double gcl_v = (wave == 0 && lane < n) ? gsh[lane] : 0.0;
    __syncthreads();
    STAMP(2);
    if (fail) {
        if (tid == 0) k5_result(st, 0, 0.0, 0.0);
        return;
    }
    bool bad = false;
    if (wave == 0) mf_factor<NF, 0>(M, Lf, Up, lane, bad);
    __syncthreads();
    mf_panel<NF, 0>(M, Lf, Up, tid, bad);
    if (wave != 0) return;
    if (bad) {
        if (lane == 0) k5_result(st, 0, 0.0, 0.0);
        return;
    }
    // z_j = L[NP][j] (row NP of the eliminated augmented matrix); L^T x = z (unit diagonal):
    // lane j, L[i][j] = Lf[j][i] column-major, zero for i <= j so the update needs no select
    const int lj = lane < NP ? lane : 0;
    double yv = lane < NP ? Lf[lj * kMfLd + NP] : 0.0;
    double lt[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const double m = Lf[lj * kMfLd + j];
        lt[j] = lane < j ? m : 0.0;
    }
#pragma unroll
    for (int j = NP - 1; j >= 0; --j) yv = fma(-lt[j], rl64(yv, j), yv);
    STAMP(3);
    k5_finish<NF>(G, Wk, Up, lane < n ? yv : 0.0, gcl_v, n, lane, p7, fidx);
    RTSTAMP(5);
}

template <int NF>
__global__ __launch_bounds__(kK5Threads) void ba_camera_solve_mfma(Geometry G, Prob Pr, Work Wk, int combine) {
    camera_solve_mfma_body<NF>(G, Pr, Wk, combine);
}

// K5 of the landmark-sharded iteration over the P2P exchange: the exchange of the reduced system
// (X1: combine + push + flags + rank-ordered sum) in the prologue, then the same factorisation
template <int NF, bool LL>
__global__ __launch_bounds__(kK5Threads) void ba_camera_solve_mfma_p2p(Geometry G, Prob Pr, Work Wk, P2P P,
                                                                        unsigned long long* xgen, int* err) {
    camera_solve_mfma_body<NF, LL>(G, Pr, Wk, 2, &P, xgen, err);
}
