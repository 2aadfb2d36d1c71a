// ba_landmarks.hpp -- device-side landmark triangulation and the depth / reprojection gate
// (rsvio_ba_triangulate, rsvio_ba_check_landmarks).  Included by ba.hip inside its file-local
// namespace: it uses that file's Geometry / Prob / SlotSrc types and the padded slot layout.
//
// The reference creates every landmark that is not in the map at depth 2.0 along the ray of its
// first observation and leaves two TODOs (src/estimator/sliding_window.rs:257 "Triangulate
// instead of assigning depth", :472 "check if points are estimated at obviously wrong
// locations"); its configs' `depth: {min_depth, max_depth}` section is read by nothing.  This is
// both: the least-squares intersection of the observation rays and, on any state, the depth and
// reprojection report per landmark.
//
// Per observation o of a slot (keyframe k, camera c, normalised (u, v)):
//   T = T_C_B[c] T_B_W(k) = [R | t],  centre c_o = -R^T t,  unit ray d_o = R^T (u, v, 1)^T / |.|,
//   M_o = I - d_o d_o^T
// per landmark  A = sum M_o,  r = sum M_o c_o,  p = A^-1 r  over the observations used
// (RSVIO_TRI_ALL_VIEWS: all; RSVIO_TRI_FIRST_STEREO: the two of the first slot holding both
// cameras).  For two rays det A = 2 sin^2(angle between them).
//
// Grid: the K4 / K6 grid -- one wave per landmark group, one lane per slot -- plus one thread per
// landmark for those without a slot (the slot-driven pass never visits them).  The per-landmark
// sums run in slot order from LDS by the landmark's first lane, as store_linearization's do: no
// floating-point atomics, two runs give the same bits.
#pragma once

struct LmGate {
    int mode;
    double min_depth, max_depth, max_sq_error;
};

// [R | t] = T_C_B[cam] T_B_W
__device__ __forceinline__ void camera_from_world(const Pose& P, const double* TCB, double R[3][3], double t[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            R[i][j] = (TCB[4 * i] * P.R[0][j] + TCB[4 * i + 1] * P.R[1][j]) + TCB[4 * i + 2] * P.R[2][j];
        t[i] = ((TCB[4 * i] * P.t[0] + TCB[4 * i + 1] * P.t[1]) + TCB[4 * i + 2] * P.t[2]) + TCB[4 * i + 3];
    }
}

// TRI: triangulate from `pose` (the initial poses) into pw_out (the initial points) for the
// landmarks `sel` selects (null = all) that pass the gate; else report on the state (pose, pw).
// sel is the handle's pinned staging itself, read over PCIe at system scope (one byte per
// landmark by its first lane, issued with the header loads): no copy precedes the kernel.
// info: one record per landmark.  blocks [0, n_wave): the slot waves; the rest: 64 landmarks each,
// those without a slot.
// bx: the block's index within its window (the grid's x; a batched grid's y is the window).
template <bool TRI>
__device__ __forceinline__ void landmarks_body(const Geometry& G, const Prob& Pr, const unsigned long long* obs_mask,
                                               const double* pose, const double* pw, double* pw_out,
                                               const unsigned char* sel, const LmGate& gate,
                                               rsvio_landmark_info* info, int bx) {
    __shared__ double shA[10][64];  // A (packed upper, 6), r (3), observations used
    __shared__ double shP[4][64];   // the landmark's point and whether it has one, at its first lane
    __shared__ double shG[3][64];   // min depth, max depth, max squared error of the slot
    const int lane = threadIdx.x;
    if (bx >= G.n_wave) {  // landmarks without a slot
        const int l = 64 * (bx - G.n_wave) + lane;
        if (l < G.n_lm && obs_mask[l] == 0ull) {
            const bool on = !TRI || !sel || __hip_atomic_load(sel + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            rsvio_landmark_info r;
            r.n_obs = 0;
            r.flags = on ? RSVIO_LM_TOO_FEW : RSVIO_LM_NOT_SELECTED;
            r.min_depth = r.max_depth = r.max_sq_error = 0.0;
            info[l] = r;
        }
        return;
    }
    const int s = 64 * bx + lane;
    const int4 h0 = Pr.slot_hdr[2 * s], h1 = Pr.slot_hdr[2 * s + 1];
    const double2 uvq[2] = {Pr.slot_uv[2 * s], Pr.slot_uv[2 * s + 1]};
    const bool act = h1.y > 0;
    const int kf = h0.x, l = h0.y, first = act ? h0.z : lane, nk = act ? h0.w : 1;
    const int nobs = h1.y, cams = h1.z;
    const bool head = act && lane == first;
    bool on = true;
    if (TRI && sel && head) on = __hip_atomic_load(sel + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
    // the observations used: all of the slot, or (first-stereo mode) both of the landmark's first
    // slot that holds two
    bool use = act;
    if (TRI && gate.mode == RSVIO_TRI_FIRST_STEREO) {
        const unsigned long long stereo = __ballot(act && nobs == 2);
        const unsigned long long seg = (nk >= 64 ? ~0ull : (1ull << nk) - 1ull) << first;
        const unsigned long long hit = stereo & seg;
        use = act && hit && lane == __ffsll((long long)hit) - 1;
    }
    const Pose P = pose_from7(pose + 7 * (act ? kf : 0));
    double R[2][3][3], t[2][3];
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0};
    int n_used = 0;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        if (o >= nobs) break;
        camera_from_world(P, G.TCB[(cams >> o) & 1].m, R[o], t[o]);
        if (!use) continue;
        const double u = uvq[o].x, v = uvq[o].y;
        double c[3], d[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            c[j] = -((R[o][0][j] * t[o][0] + R[o][1][j] * t[o][1]) + R[o][2][j] * t[o][2]);
            d[j] = (R[o][0][j] * u + R[o][1][j] * v) + R[o][2][j];
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
        ++n_used;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) shA[i][lane] = A[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) shA[6 + i][lane] = r[i];
    shA[9][lane] = (double)n_used;
    __syncthreads();
    int n = 0, flags = 0;
    double p[3] = {0.0, 0.0, 0.0};
    if (head) {  // the landmark's sums in slot order, then the 3x3 solve
        double Al[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, rl[3] = {0.0, 0.0, 0.0}, nl = 0.0;
        for (int k = 0; k < nk; ++k) {
#pragma unroll
            for (int i = 0; i < 6; ++i) Al[i] += shA[i][first + k];
#pragma unroll
            for (int i = 0; i < 3; ++i) rl[i] += shA[6 + i][first + k];
            nl += shA[9][first + k];
        }
        n = (int)nl;
        if (!TRI) {  // the state's own point
            p[0] = pw[3 * l];
            p[1] = pw[3 * l + 1];
            p[2] = pw[3 * l + 2];
        } else if (n < 2) {
            flags = RSVIO_LM_TOO_FEW;
        } else {
            const double c00 = Al[3] * Al[5] - Al[4] * Al[4];
            const double c01 = Al[4] * Al[2] - Al[1] * Al[5];
            const double c02 = Al[1] * Al[4] - Al[3] * Al[2];
            const double det = (Al[0] * c00 + Al[1] * c01) + Al[2] * c02;
            if (!(det > 1e-12 * (nl * nl * nl)) || !isfinite(det)) {
                flags = RSVIO_LM_DEGENERATE;
            } else {
                const double id = 1.0 / det;
                const double c11 = Al[0] * Al[5] - Al[2] * Al[2];
                const double c12 = Al[1] * Al[2] - Al[0] * Al[4];
                const double c22 = Al[0] * Al[3] - Al[1] * Al[1];
                p[0] = ((c00 * rl[0] + c01 * rl[1]) + c02 * rl[2]) * id;
                p[1] = ((c01 * rl[0] + c11 * rl[1]) + c12 * rl[2]) * id;
                p[2] = ((c02 * rl[0] + c12 * rl[1]) + c22 * rl[2]) * id;
            }
        }
        shP[0][lane] = p[0];
        shP[1][lane] = p[1];
        shP[2][lane] = p[2];
        shP[3][lane] = flags ? 0.0 : 1.0;
    }
    __syncthreads();
    // the gate: depth and squared normalised reprojection error of every observation used
    double zmin = INFINITY, zmax = -INFINITY, emax = 0.0;
    if (use && shP[3][first] != 0.0) {
        const double q[3] = {shP[0][first], shP[1][first], shP[2][first]};
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            if (o >= nobs) break;
            double pc[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) pc[i] = ((R[o][i][0] * q[0] + R[o][i][1] * q[1]) + R[o][i][2] * q[2]) + t[o][i];
            const double e0 = pc[0] / pc[2] - uvq[o].x, e1 = pc[1] / pc[2] - uvq[o].y;
            const double e = e0 * e0 + e1 * e1;
            zmin = pc[2] < zmin ? pc[2] : zmin;
            zmax = pc[2] > zmax ? pc[2] : zmax;
            emax = e > emax ? e : emax;
        }
    }
    shG[0][lane] = zmin;
    shG[1][lane] = zmax;
    shG[2][lane] = emax;
    __syncthreads();
    if (!head) return;
    rsvio_landmark_info out;
    out.n_obs = 0;
    out.flags = RSVIO_LM_NOT_SELECTED;
    out.min_depth = out.max_depth = out.max_sq_error = 0.0;
    if (on) {
        out.n_obs = n;
        if (!flags) {
            zmin = INFINITY, zmax = -INFINITY, emax = 0.0;
            for (int k = 0; k < nk; ++k) {
                const double a = shG[0][first + k], b = shG[1][first + k], e = shG[2][first + k];
                zmin = a < zmin ? a : zmin;
                zmax = b > zmax ? b : zmax;
                emax = e > emax ? e : emax;
            }
            if (zmin < gate.min_depth || zmax > gate.max_depth) flags |= RSVIO_LM_DEPTH;
            if (gate.max_sq_error > 0.0 && emax > gate.max_sq_error) flags |= RSVIO_LM_ERROR;
            if (!flags) flags = RSVIO_LM_OK;
            out.min_depth = zmin;
            out.max_depth = zmax;
            out.max_sq_error = emax;
        }
        out.flags = flags;
        if (TRI && flags == RSVIO_LM_OK) {
            pw_out[3 * l] = p[0];
            pw_out[3 * l + 1] = p[1];
            pw_out[3 * l + 2] = p[2];
        }
    }
    info[l] = out;
}

template <bool TRI>
__global__ __launch_bounds__(64) void ba_landmarks(Geometry G, Prob Pr, const unsigned long long* obs_mask,
                                                   const double* pose, const double* pw, double* pw_out,
                                                   const unsigned char* sel, LmGate gate,
                                                   rsvio_landmark_info* info) {
    landmarks_body<TRI>(G, Pr, obs_mask, pose, pw, pw_out, sel, gate, info, (int)blockIdx.x);
}

// Batched mode (rsvio_ba_batch_triangulate / _check_landmarks): one row per window, everything
// the single kernel takes by value.  Grid (max over the active windows of n_wave +
// ceil(n_lm / 64), B); a block past its window's bound, or of an inactive window, returns whole
// before the body's first barrier.  The gate is the row's: two windows of one call may differ.
struct LmDesc {
    Geometry G;
    Prob Pr;
    const unsigned long long* obs_mask;
    const double* pose;   // the state the single call would read: the initial poses (triangulate),
    const double* pw;     // or what get_state would return (check)
    double* pw_out;       // the arena's initial point array
    const unsigned char* sel;
    LmGate gate;
    rsvio_landmark_info* info;
    int skip;
};

template <bool TRI>
__global__ __launch_bounds__(64) void bab_landmarks(const LmDesc* __restrict__ D) {
    const LmDesc& d = D[blockIdx.y];
    const int skip = d.skip, bound = d.G.n_wave + (d.G.n_lm + 63) / 64;
    const Prob Pr = d.Pr;
    const unsigned long long* obs_mask = d.obs_mask;
    const double* pose = d.pose;
    desc_touch(Pr.slot_hdr, Pr.slot_uv, obs_mask, pose);
    if (skip | ((int)blockIdx.x >= bound)) return;
    landmarks_body<TRI>(d.G, Pr, obs_mask, pose, d.pw, d.pw_out, d.sel, d.gate, d.info, (int)blockIdx.x);
}
