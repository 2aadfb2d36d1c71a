// pnp_robust.hpp -- outlier-robust motion tracking: a stereo 3-point RANSAC in front of the PnP LM
// (rsvio_track_motion_robust*).  Included by pnp.hip inside its file-local namespace, after
// pnp_track_motion_kernel: it reuses that file's PnpArgs, map_lookup and pnp_finish, and its refit
// runs that file's LM -- LmLds, prior_pose, ctl_start, ctl_publish, tcw_entry and lm_passes, the one
// pass loop there is -- so the two cannot drift apart.
//
// Three launches on the handle's stream, no host wait between them and no workgroup waiting on
// another (no spin flag, no last-block reducer): what one launch reduces, the next one reads.
//   R1 pnp_robust_join_kernel    one workgroup: the map join of both feature lists, compacted in
//      list order (left, then right) into a structure of arrays in global memory; the stereo
//      pairs (an id in both lists with a map point, by ascending left position) through an LDS
//      hash of the right list; each pair's point q in the BODY frame by ba_landmarks.hpp's
//      least-squares ray intersection at T_B_W = I.
//   R2 pnp_robust_score_kernel   one wave per hypothesis: h = 0 the prior (the pose the plain LM
//      starts from), h >= 1 the rigid motion between a world and a body triangle of three pairs;
//      the inliers over all joined observations by ballot / popcount (integers: order-free).
//   R3 pnp_robust_refit_kernel   one workgroup: the winner (largest count, lowest h on a tie),
//      the plain kernel's LM (lm_passes) on the winner's inliers from the winner's pose -- the
//      same function over the same factor order and lane <-> feature assignment, so n_hyp = 1 with
//      an all-accepting threshold gives the plain kernel's bits -- then the inlier / outlier mask
//      of every joined observation at the refined pose.
#pragma once

constexpr int kRansacMaxHyp = 1024;

struct RobustBufs {
    double* w;         // [3][kPnpMaxFeatures]  the joined observations: map point (f32 widened)
    double* uv;        // [2][kPnpMaxFeatures]  ... undistorted coordinates (f32 widened)
    int* cam;          // ... camera
    int* pos;          // ... position in the caller's list of that camera
    double* pair_q;    // [3][kPnpMaxFeatures]  the pairs: point in the body frame
    double* pair_w;    // [3][kPnpMaxFeatures]  ... map point
    int* pair_ok;      // ... valid
    int* counts;       // n_obs, n_pairs, n_valid_pairs
    double* hyp_pose;  // [kRansacMaxHyp][12]  R_BW (row-major), t_BW
    int* hyp_count;    // [kRansacMaxHyp]      inliers, -1: invalid
    const int* samples;  // [n_hyp][3] pair indices, or null: the seeded sampler
    uint8_t* mask;     // [n_l + n_r]  0 no map point, 1 inlier, 2 outlier
};

struct RobustArgs {
    PnpArgs P;  // P.out: the motion member of *out
    RobustBufs B;
    int n_hyp, min_inliers;
    uint64_t seed;
    double inlier_sq, min_depth;
    rsvio_robust_motion_result* out;  // pinned host memory
};

// One stream's scratch as the host allocates it: RobustBufs' f64 arrays in one buffer (w, uv,
// pair_q, pair_w, hyp_pose), cam, pos, pair_ok and counts (4) in another; hyp_count, samples and
// mask are placed by the caller
constexpr size_t kRobustDbl = (3 + 2 + 3 + 3) * (size_t)kPnpMaxFeatures + 12 * (size_t)kRansacMaxHyp;
constexpr size_t kRobustInt = 3 * (size_t)kPnpMaxFeatures + 4;

RobustBufs robust_carve(double* d, int* q) {
    constexpr size_t cap = kPnpMaxFeatures;
    RobustBufs B{};
    B.w = d;
    B.uv = B.w + 3 * cap;
    B.pair_q = B.uv + 2 * cap;
    B.pair_w = B.pair_q + 3 * cap;
    B.hyp_pose = B.pair_w + 3 * cap;
    B.cam = q;
    B.pos = B.cam + cap;
    B.pair_ok = B.pos + cap;
    B.counts = B.pair_ok + cap;
    return B;
}

void set_ransac(RobustArgs& RA, const rsvio_ransac_cfg* rc) {
    RA.n_hyp = rc->n_hyp;
    RA.min_inliers = rc->min_inliers;
    RA.seed = rc->seed;
    RA.inlier_sq = rc->inlier_sq_error;
    RA.min_depth = rc->min_depth;
}

__host__ __device__ __forceinline__ uint64_t splitmix64_at(uint64_t seed, uint64_t i) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (i + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// T_C_W = T_C_B [R | t] as 12 values (R row-major, then t) by one thread, R and t apart: pnp.hip's
// tcw_entry for all 12 entries (written out: through tcw_entry R2's schedule changes)
__device__ __forceinline__ void compose_tcw(const double* T, const double* R, const double* t, double* out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) out[3 * i + j] = (T[4 * i] * R[j] + T[4 * i + 1] * R[3 + j]) + T[4 * i + 2] * R[6 + j];
        out[9 + i] = ((T[4 * i] * t[0] + T[4 * i + 1] * t[1]) + T[4 * i + 2] * t[2]) + T[4 * i + 3];
    }
}

// The inlier test of R2 and R3 (one function: both take the same decision on the same input):
// p_C = T_C_W p_W in front of the camera by min_depth and within the squared error
__device__ __forceinline__ bool robust_inlier(const double* T0, const double* T1, int cam, const double w[3],
                                              const double uv[2], double min_depth, double sq) {
    double T[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = cam ? T1[e] : T0[e];
    const double x = ((T[0] * w[0] + T[1] * w[1]) + T[2] * w[2]) + T[9];
    const double y = ((T[3] * w[0] + T[4] * w[1]) + T[5] * w[2]) + T[10];
    const double z = ((T[6] * w[0] + T[7] * w[1]) + T[8] * w[2]) + T[11];
    const double e0 = x / z - uv[0], e1 = y / z - uv[1];
    return z >= min_depth && (e0 * e0 + e1 * e1) <= sq;
}

// ba_landmarks.hpp's two-ray intersection at T_B_W = I: [R | t] = T_C_B[c]; valid iff
// det A > 1e-12 2^3, q finite and both depths >= min_depth
__device__ __forceinline__ bool pair_triangulate(const double* TCB /* [2][16] */, const double u[2], const double v[2],
                                                 double min_depth, double q[3]) {
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        const double* T = TCB + 16 * o;
        double c[3], d[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            c[j] = -((T[j] * T[3] + T[4 + j] * T[7]) + T[8 + j] * T[11]);
            d[j] = (T[j] * u[o] + T[4 + j] * v[o]) + T[8 + j];
        }
        const double in = 1.0 / sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
        for (int j = 0; j < 3; ++j) d[j] *= in;
        const double dc = (d[0] * c[0] + d[1] * c[1]) + d[2] * c[2];
        A[0] += 1.0 - d[0] * d[0];
        A[1] += -d[0] * d[1];
        A[2] += -d[0] * d[2];
        A[3] += 1.0 - d[1] * d[1];
        A[4] += -d[1] * d[2];
        A[5] += 1.0 - d[2] * d[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) r[j] += c[j] - d[j] * dc;
    }
    const double c00 = A[3] * A[5] - A[4] * A[4];
    const double c01 = A[4] * A[2] - A[1] * A[5];
    const double c02 = A[1] * A[4] - A[3] * A[2];
    const double det = (A[0] * c00 + A[1] * c01) + A[2] * c02;
    q[0] = q[1] = q[2] = 0.0;
    if (!(det > 1e-12 * 8.0) || !isfinite(det)) return false;
    const double id = 1.0 / det;
    const double c11 = A[0] * A[5] - A[2] * A[2];
    const double c12 = A[1] * A[2] - A[0] * A[4];
    const double c22 = A[0] * A[3] - A[1] * A[1];
    q[0] = ((c00 * r[0] + c01 * r[1]) + c02 * r[2]) * id;
    q[1] = ((c01 * r[0] + c11 * r[1]) + c12 * r[2]) * id;
    q[2] = ((c02 * r[0] + c12 * r[1]) + c22 * r[2]) * id;
    if (!(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))) return false;
    bool ok = true;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        const double* T = TCB + 16 * o;
        const double z = ((T[8] * q[0] + T[9] * q[1]) + T[10] * q[2]) + T[11];
        ok &= z >= min_depth;
    }
    return ok;
}

// Exclusive scan of one int per thread over the workgroup, in thread order; *total: the sum
__device__ __forceinline__ int block_excl_scan(int v, int* s_w, int tid, int* total) {
    const int lane = tid & 63, wv = tid >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    __syncthreads();  // s_w's previous readers
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kPnpWaves; ++w) {
        const int x = s_w[w];
        tot += x;
        base += w < wv ? x : 0;
    }
    *total = tot;
    return base + inc - v;
}

template <int CAP>
__device__ __forceinline__ uint32_t pair_slot(uint64_t id) {
    return (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> 51) & (uint32_t)(2 * CAP - 1);
}

__device__ __forceinline__ uint64_t feature_id(const PnpArgs& A, int cam, int i) {
    return *reinterpret_cast<const uint64_t*>(A.ids[cam] + (size_t)i * A.id_stride);
}

// R1: join, pair and triangulate.  One workgroup; feature j of the combined list (left then right)
// lives at LDS entry j as in the plain kernel.  The bodies of R1 to R3 are shared by the
// single-stream kernels (RA by value) and the batched ones (RA in a device table); CAP is the LDS
// capacity in features (nf <= CAP, checked on the host), `cap` the stride of the global arrays,
// which does not depend on it.  The pairs come out by ascending left position whatever slot of
// the LDS hash an id takes, so CAP changes no result.
template <int CAP>
__device__ __forceinline__ void pnp_robust_join_body(const RobustArgs& RA) {
    constexpr int kPairSlots = 2 * CAP;         // LDS hash of the right list: load <= 1/2
    __shared__ float s_mpw[3][CAP];
    __shared__ float s_uv[2][CAP];
    __shared__ int8_t s_cam[CAP];               // feature -> camera, -1: no map point
    __shared__ short s_mate[CAP];               // left feature -> its id's position in the right list, -1: none
    __shared__ int s_ht[kPairSlots];            // hash of the joined right features: position, -1: free
    __shared__ int s_w[kPnpWaves];
    __shared__ int s_nvalid;
    const PnpArgs& A = RA.P;
    const int tid = threadIdx.x;
    const int n0 = A.n[0], n1 = A.n[1], nf = n0 + n1;  // nf <= CAP (checked on the host)
    constexpr int cap = kPnpMaxFeatures;
    for (int s = tid; s < kPairSlots; s += kPnpThreads) s_ht[s] = -1;
    for (int j = tid; j < CAP; j += kPnpThreads) {
        s_mate[j] = -1;
        s_cam[j] = -1;
    }
    if (tid == 0) s_nvalid = 0;
    __syncthreads();
    // the join; a joined right feature enters the hash (equal ids keep the lowest position)
    for (int j = tid; j < nf; j += kPnpThreads) {
        const int cam = j < n0 ? 0 : 1;
        const int i = cam == 0 ? j : j - n0;
        const uint64_t id = feature_id(A, cam, i);
        const float2 q = A.uv[cam][i];
        float pw[3];
        const bool hit = A.n_map > 0 && map_lookup(A, id, pw);
        if (!hit) continue;
        s_cam[j] = (int8_t)cam;
        s_uv[0][j] = q.x;
        s_uv[1][j] = q.y;
        s_mpw[0][j] = pw[0];
        s_mpw[1][j] = pw[1];
        s_mpw[2][j] = pw[2];
        if (cam == 1) {
            uint32_t s = pair_slot<CAP>(id);
            for (int probe = 0; probe < kPairSlots; ++probe) {
                const int prev = atomicCAS(&s_ht[s], -1, i);
                if (prev == -1) break;
                if (feature_id(A, 1, prev) == id) {
                    atomicMin(&s_ht[s], i);
                    break;
                }
                s = (s + 1) & (uint32_t)(kPairSlots - 1);
            }
        }
    }
    __syncthreads();
    for (int j = tid; j < n0; j += kPnpThreads) {
        if (s_cam[j] < 0) continue;
        const uint64_t id = feature_id(A, 0, j);
        uint32_t s = pair_slot<CAP>(id);
        for (int probe = 0; probe < kPairSlots; ++probe) {
            const int at = s_ht[s];
            if (at < 0) break;
            if (feature_id(A, 1, at) == id) {
                s_mate[j] = (short)at;
                break;
            }
            s = (s + 1) & (uint32_t)(kPairSlots - 1);
        }
    }
    __syncthreads();
    // compaction in list order: thread t owns features [kChunk t, kChunk (t + 1))
    constexpr int kChunk = CAP / kPnpThreads;
    const int j_lo = tid * kChunk;
    int c_obs = 0, c_pair = 0;
#pragma unroll
    for (int e = 0; e < kChunk; ++e) {
        const int j = j_lo + e;
        c_obs += s_cam[j] >= 0 ? 1 : 0;
        c_pair += (j < n0 && s_cam[j] >= 0 && s_mate[j] >= 0) ? 1 : 0;
    }
    int n_obs, n_pairs;
    int k = block_excl_scan(c_obs, s_w, tid, &n_obs);
    int p = block_excl_scan(c_pair, s_w, tid, &n_pairs);
    int valid = 0;
    for (int e = 0; e < kChunk; ++e) {
        const int j = j_lo + e;
        const int cam = s_cam[j];
        if (cam < 0) continue;
        const double w[3] = {(double)s_mpw[0][j], (double)s_mpw[1][j], (double)s_mpw[2][j]};
        RA.B.w[k] = w[0];
        RA.B.w[cap + k] = w[1];
        RA.B.w[2 * cap + k] = w[2];
        RA.B.uv[k] = (double)s_uv[0][j];
        RA.B.uv[cap + k] = (double)s_uv[1][j];
        RA.B.cam[k] = cam;
        RA.B.pos[k] = cam == 0 ? j : j - n0;
        ++k;
        if (j >= n0 || s_mate[j] < 0) continue;
        const int jr = n0 + s_mate[j];
        const double u[2] = {(double)s_uv[0][j], (double)s_uv[0][jr]};
        const double v[2] = {(double)s_uv[1][j], (double)s_uv[1][jr]};
        double q[3];
        const bool ok = pair_triangulate(&A.TCB[0][0], u, v, RA.min_depth, q);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            RA.B.pair_q[c * cap + p] = q[c];
            RA.B.pair_w[c * cap + p] = w[c];
        }
        RA.B.pair_ok[p] = ok ? 1 : 0;
        valid += ok ? 1 : 0;
        ++p;
    }
    if (valid) atomicAdd(&s_nvalid, valid);
    __syncthreads();
    if (tid == 0) {
        RA.B.counts[0] = n_obs;
        RA.B.counts[1] = n_pairs;
        RA.B.counts[2] = s_nvalid;
    }
}

__global__ __launch_bounds__(kPnpThreads) void pnp_robust_join_kernel(RobustArgs RA) {
    pnp_robust_join_body<kPnpMaxFeatures>(RA);
}

// Batched R1: workgroup blockIdx.x is stream i
template <int CAP>
__global__ __launch_bounds__(kPnpThreads) void pnp_robust_join_batch_kernel(const RobustArgs* __restrict__ table) {
    pnp_robust_join_body<CAP>(table[blockIdx.x]);
}

// The orthonormal frame of a triangle (columns e1, e2, e3 in F[3 i + c]) and its centroid; false
// when the triangle is degenerate: |a x b|^2 <= 1e-12 |a|^2 |b|^2
__device__ __forceinline__ bool triangle_frame(const double p[3][3], double F[9], double mean[3]) {
    double a[3], b[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a[i] = p[1][i] - p[0][i];
        b[i] = p[2][i] - p[0][i];
        mean[i] = ((p[0][i] + p[1][i]) + p[2][i]) / 3.0;
    }
    const double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    const double bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (!(nn > 1e-12 * (aa * bb))) return false;
    const double ia = 1.0 / sqrt(aa), in = 1.0 / sqrt(nn);
    double e1[3], e3[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        e1[i] = a[i] * ia;
        e3[i] = n[i] * in;
    }
    const double e2[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        F[3 * i] = e1[i];
        F[3 * i + 1] = e2[i];
        F[3 * i + 2] = e3[i];
    }
    return true;
}

// R2: one wave per hypothesis (blockIdx.x)
__device__ __forceinline__ void pnp_robust_score_body(const RobustArgs& RA) {
    const PnpArgs& A = RA.P;
    const int h = blockIdx.x, lane = threadIdx.x;
    constexpr int cap = kPnpMaxFeatures;
    const int n_obs = RA.B.counts[0], n_pairs = RA.B.counts[1];
    double R[9], t[3];
    bool ok = true;
    if (h == 0) {
        double x[7];
        prior_pose(A, x, R);
        t[0] = x[0];
        t[1] = x[1];
        t[2] = x[2];
    } else {
        int idx[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (RA.B.samples)
                idx[k] = RA.B.samples[3 * h + k];
            else
                idx[k] = n_pairs > 0 ? (int)(splitmix64_at(RA.seed, (uint64_t)(3 * h + k)) % (uint64_t)n_pairs) : -1;
        }
        ok = n_pairs >= 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) ok &= idx[k] >= 0 && idx[k] < n_pairs;
        ok = ok && idx[0] != idx[1] && idx[0] != idx[2] && idx[1] != idx[2];
        double pw[3][3], pq[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = ok ? idx[k] : 0;  // (slot 0 exists: never dereferenced past the buffers)
            ok = ok && RA.B.pair_ok[i] != 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                pw[k][c] = RA.B.pair_w[c * cap + i];
                pq[k][c] = RA.B.pair_q[c * cap + i];
            }
        }
        double Fw[9], Fq[9], mw[3], mq[3];
        const bool fw = triangle_frame(pw, Fw, mw), fq = triangle_frame(pq, Fq, mq);
        ok = ok && fw && fq;
        if (ok) {
            // R = F_q F_w^T, t = mean(q) - R mean(w)
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    R[3 * i + j] = (Fq[3 * i] * Fw[3 * j] + Fq[3 * i + 1] * Fw[3 * j + 1]) + Fq[3 * i + 2] * Fw[3 * j + 2];
#pragma unroll
            for (int i = 0; i < 3; ++i) t[i] = mq[i] - ((R[3 * i] * mw[0] + R[3 * i + 1] * mw[1]) + R[3 * i + 2] * mw[2]);
#pragma unroll
            for (int k = 0; k < 9; ++k) ok &= isfinite(R[k]);
#pragma unroll
            for (int k = 0; k < 3; ++k) ok &= isfinite(t[k]);
        }
        if (!ok) {
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
            t[0] = t[1] = t[2] = 0.0;
        }
    }
    int count = -1;
    if (ok) {  // (uniform over the wave)
        double T0[12], T1[12];
        compose_tcw(A.TCB[0], R, t, T0);
        compose_tcw(A.TCB[1], R, t, T1);
        count = 0;
        for (int k0 = 0; k0 < n_obs; k0 += 64) {
            const int k = k0 + lane;
            bool in = false;
            if (k < n_obs) {
                const double w[3] = {RA.B.w[k], RA.B.w[cap + k], RA.B.w[2 * cap + k]};
                const double uv[2] = {RA.B.uv[k], RA.B.uv[cap + k]};
                in = robust_inlier(T0, T1, RA.B.cam[k], w, uv, RA.min_depth, RA.inlier_sq);
            }
            count += __popcll(__ballot(in));
        }
    }
    if (lane == 0) {
        RA.B.hyp_count[h] = count;
#pragma unroll
        for (int k = 0; k < 9; ++k) RA.B.hyp_pose[12 * h + k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) RA.B.hyp_pose[12 * h + 9 + k] = t[k];
    }
}

__global__ __launch_bounds__(64) void pnp_robust_score_kernel(RobustArgs RA) { pnp_robust_score_body(RA); }

// Batched R2 on a grid of (n_hyp, n): blockIdx.x the hypothesis, blockIdx.y the stream
__global__ __launch_bounds__(64) void pnp_robust_score_batch_kernel(const RobustArgs* __restrict__ table) {
    pnp_robust_score_body(table[blockIdx.y]);
}

// Unit quaternion (w, i, j, k; w >= 0) of a rotation matrix, by its largest diagonal form
__device__ __forceinline__ void quat_of_rotation(const double* R, double* q) {
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0.0) {
        const double s = 2.0 * sqrt(tr + 1.0);
        q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
        q[0] = (R[7] - R[5]) / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
        const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
        q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s;
    } else {
        const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
        q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s;
    }
    if (q[0] < 0.0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = -q[k];
    }
}

// R3: select, refit, classify.  One workgroup; the LM is the plain kernel's (ctl_start,
// ctl_publish, tcw_entry and lm_passes of pnp.hip, without the stamps) over the LDS entries of the
// winner's inliers: a feature that is no inlier, or has no map point, is no factor.
template <int CAP>
__device__ __forceinline__ void pnp_robust_refit_body(const RobustArgs& RA) {
    __shared__ LmLds<CAP> S;
    __shared__ uint8_t s_mask[CAP];
    __shared__ double s_tcw0[2][12];              // T_C_W at the winner's pose
    __shared__ long long s_key[kPnpWaves];
    __shared__ int s_nvalid[kPnpWaves];
    __shared__ int s_nin;
    const PnpArgs& A = RA.P;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr int cap = kPnpMaxFeatures;
    const unsigned long long t_entry = wall_clock64();
    const int n0 = A.n[0], nf = n0 + A.n[1];
    const int n_obs = RA.B.counts[0];
    // the winner: the largest count, the lowest h on a tie -- the maximum of count 2^11 + (1023 - h)
    long long key = -1;
    int nvalid = 0;
    for (int h = tid; h < RA.n_hyp; h += kPnpThreads) {
        const int c = RA.B.hyp_count[h];
        if (c < 0) continue;
        ++nvalid;
        const long long kk = ((long long)c << 11) | (long long)(kRansacMaxHyp - 1 - h);
        key = kk > key ? kk : key;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const long long o = __shfl_xor(key, off);
        key = o > key ? o : key;
        nvalid += __shfl_xor(nvalid, off);
    }
    if (lane == 0) {
        s_key[wv] = key;
        s_nvalid[wv] = nvalid;
    }
    if (tid == 0) {
        S.s_nobs = 0;
        s_nin = 0;
    }
    if (tid < 32) S.s_tcb[tid >> 4][tid & 15] = A.TCB[tid >> 4][tid & 15];
    for (int j = tid; j < CAP; j += kPnpThreads) {
        S.s_cam[j] = -1;
        s_mask[j] = 0;
    }
    __syncthreads();
    key = s_key[0];
    nvalid = s_nvalid[0];
#pragma unroll
    for (int w = 1; w < kPnpWaves; ++w) {
        key = s_key[w] > key ? s_key[w] : key;
        nvalid += s_nvalid[w];
    }
    const int best_h = key < 0 ? -1 : kRansacMaxHyp - 1 - (int)(key & (kRansacMaxHyp - 1));
    const int best_count = key < 0 ? -1 : (int)(key >> 11);
    const int need = RA.min_inliers > 1 ? RA.min_inliers : 1;
    const bool consensus = best_count >= need;
    // wave 0: the LM state, F starting from the winner's pose (h = 0: the plain kernel's start)
    if (wv == 0) {
        Ctl C;
        ctl_start(A, C);
        if (best_h <= 0) {
            prior_pose(A, C.x, C.R);
        } else {
            const double* hp = RA.B.hyp_pose + 12 * best_h;
            double Rw[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) Rw[k] = hp[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) C.x[k] = hp[9 + k];
            quat_of_rotation(Rw, C.x + 3);
            const Pose P0 = pose_from7(C.x);
#pragma unroll
            for (int k = 0; k < 9; ++k) C.R[k] = P0.R[k / 3][k % 3];
        }
        if (lane == 0) ctl_publish(C, S.s_pose, S.s_ctl);
    }
    __syncthreads();  // s_tcb, s_pose
    if (wv == 0 && lane < 24) {
        const int c = lane / 12, e = lane % 12;
        const double v = tcw_entry(S.s_tcb[c], S.s_pose, e);
        S.s_tcw[c][e] = v;
        s_tcw0[c][e] = v;
    }
    __syncthreads();  // the winner's T_C_W
    // the factor list: the winner's inliers, each at its feature's LDS entry
    int mine = 0;
    for (int k = tid; k < n_obs && consensus; k += kPnpThreads) {
        const double w[3] = {RA.B.w[k], RA.B.w[cap + k], RA.B.w[2 * cap + k]};
        const double uv[2] = {RA.B.uv[k], RA.B.uv[cap + k]};
        const int cam = RA.B.cam[k];
        if (!robust_inlier(s_tcw0[0], s_tcw0[1], cam, w, uv, RA.min_depth, RA.inlier_sq)) continue;
        const int j = cam == 0 ? RA.B.pos[k] : n0 + RA.B.pos[k];
        S.s_cam[j] = (int8_t)cam;
        S.s_uv[0][j] = (float)uv[0];
        S.s_uv[1][j] = (float)uv[1];
        S.s_mpw[0][j] = (float)w[0];
        S.s_mpw[1][j] = (float)w[1];
        S.s_mpw[2][j] = (float)w[2];
        ++mine;
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if (lane == 0 && mine) atomicAdd(&S.s_nobs, mine);
    __syncthreads();  // the factor list and s_nobs
    const int nobs = S.s_nobs;
    const int run = (consensus && nobs > 0) ? 1 : 0;
    if (tid == 0) {
        S.s_ctl.n_obs = run ? nobs : 0;
        if (!run) S.s_ctl.status = LM_SKIPPED;
    }
    lm_passes<false>(A, S, nf, run);
    // the mask at the refined pose (a failed LM: at the winner's); without consensus every joined
    // observation is an outlier
    __syncthreads();
    const bool refined = S.s_ctl.status > 0;
    if (tid == 0 && refined) {
        const Pose P = pose_from7(S.s_ctl.x);
#pragma unroll
        for (int k = 0; k < 9; ++k) S.s_pose[k] = P.R[k / 3][k % 3];
#pragma unroll
        for (int k = 0; k < 3; ++k) S.s_pose[9 + k] = S.s_ctl.x[k];
    }
    __syncthreads();
    if (tid < 24) {
        const int c = tid / 12, e = tid % 12;
        S.s_tcw[c][e] = refined ? tcw_entry(S.s_tcb[c], S.s_pose, e) : s_tcw0[c][e];
    }
    __syncthreads();
    int nin = 0;
    for (int k = tid; k < n_obs; k += kPnpThreads) {
        const double w[3] = {RA.B.w[k], RA.B.w[cap + k], RA.B.w[2 * cap + k]};
        const double uv[2] = {RA.B.uv[k], RA.B.uv[cap + k]};
        const int cam = RA.B.cam[k];
        const bool in = consensus && robust_inlier(S.s_tcw[0], S.s_tcw[1], cam, w, uv, RA.min_depth, RA.inlier_sq);
        const int j = cam == 0 ? RA.B.pos[k] : n0 + RA.B.pos[k];
        s_mask[j] = in ? 1 : 2;
        nin += in ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) nin += __shfl_xor(nin, off);
    if (lane == 0 && nin) atomicAdd(&s_nin, nin);
    __syncthreads();
    for (int j = tid; j < nf; j += kPnpThreads) RA.B.mask[j] = s_mask[j];
    if (tid == 0) {
        pnp_finish(A, S.s_ctl, t_entry);  // -> RA.out->motion
        rsvio_robust_motion_result* o = RA.out;
        const int n_pairs = RA.B.counts[1];
        o->ransac_status = !consensus ? RSVIO_RANSAC_NO_CONSENSUS
                                      : (n_pairs < 3 ? RSVIO_RANSAC_TOO_FEW_PAIRS : RSVIO_RANSAC_OK);
        o->n_pairs = n_pairs;
        o->n_valid_pairs = RA.B.counts[2];
        o->n_valid_hyp = nvalid;
        o->best_hyp = best_h;
        o->best_count = best_count;
        o->n_inliers = s_nin;
        o->reserved = 0;
        o->device_ms = 0.0;  // the host fills it from its events
    }
}

__global__ __launch_bounds__(kPnpThreads) void pnp_robust_refit_kernel(RobustArgs RA) {
    pnp_robust_refit_body<kPnpMaxFeatures>(RA);
}

// Batched R3: workgroup blockIdx.x is stream i
template <int CAP>
__global__ __launch_bounds__(kPnpThreads) void pnp_robust_refit_batch_kernel(const RobustArgs* __restrict__ table) {
    pnp_robust_refit_body<CAP>(table[blockIdx.x]);
}
