// pnp.hip -- B8: SlidingWindow::track_motion + the estimator's keyframe rule on gfx950 (f64).
//
// Replaces, per frame once the window is full (src/estimator/estimator.rs:195-234):
//   * the initial pose from the last keyframe, T_B_W = inv(T_W_B), q = from_matrix(R_B_W)
//     (src/estimator/sliding_window.rs:506-517);
//   * the factor list: every left then right feature whose id is in map_points gives one
//     PnPFactor (:519-547; src/optimization/factors.rs:455-583 -- no cheirality guard, 2x6
//     Jacobian [dt | dw]) with Huber(2.0);
//   * apex LM, SparseCholesky, 10 iterations, tolerances 1e-6 / 1e-9 (:494-501) -- the
//     build's LM restatement, here on a dense 6x6 system;
//   * success test (:384-395), T_W_B = inv(SE3(F)) (:566-569);
//   * the keyframe rule: T_rel = T_W_B inv(T_W_B_last_kf), ||t_rel|| > thr_t or
//     ||euler(from_matrix(R_rel))|| > thr_r (estimator.rs:201-225); on failure the frame keeps
//     is_keyframe = true and T_W_B = I (estimator.rs:228-234, frame.rs:95, state.rs:26).
//
// One workgroup of 512 lanes runs the whole sequence in one launch (no host round trip, no
// grid-wide synchronisation).  Round 6 layout:
//   * the join: rsvio_pnp_set_map builds a bucketed hash table of the map on the host (4 entries of
//     {id, p_W} per 128-B bucket, load <= 1/4) and uploads it once per map; a feature's id is looked
//     up with ONE bucket load (its map point inside the entry), so a frame pays two dependent round
//     trips (feature, bucket) instead of staging the map in LDS and an 11-step binary search
//     (10.1k of the kernel's 53.8k cycles, profiles/r05pnp_stamps.txt);
//   * the LM control runs on all of wave 0 at once, its state in registers (every lane the same
//     values) instead of lane 0 against an LDS struct; T_C_W of the next pass is written by the
//     same wave, so a pass costs two workgroup barriers instead of four.
// Every pass linearises all matched observations at one pose and reduces H (21), g (6) and the
// cost in a fixed order (DPP reduce-scatter per wave, then the waves in order).  Each pass after
// the first is at a trial pose: if the step is accepted its H and g are the next system, so an
// accepted iteration costs one pass.
//
// One translation unit: pnp_robust.hpp (the RANSAC in front of this LM) and pnp_covariance.hpp are
// fragments of it, included inside the file-local namespace after the plain kernel.  What the plain
// kernel and the robust refit share exists once, here: the LDS of one LM (LmLds<CAP>), the start
// (prior_pose, ctl_start, ctl_publish), the per-lane T_C_W entry (tcw_entry) and the whole pass loop
// (lm_passes, the plain kernel's stamps behind a template flag), besides pnp_control and pnp_finish.
// On the host the entry points share one frame packer and list setter (pack_frame, packed_lists), one
// timed section (timed_section), and the batched calls one slot check (batch_check) and one launch
// site per kernel (with_cap picks the LDS capacity).
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "rotation.hpp"
#include "se3.hpp"

namespace rsvio {
namespace {

RSVIO_DBG_DECL

constexpr int kPnpThreads = 512;
constexpr int kPnpWaves = kPnpThreads / 64;
constexpr int kPnpMaxFeatures = 4096; // features per frame (both cameras), observations in LDS
constexpr int kRed = 28;          // H upper (21), g (6), cost
constexpr uint64_t kEmptyId = ~0ull;  // a free hash-table entry
constexpr int kBucket = 4;            // entries per 128-B bucket

// One hash-table entry: the map id and its point (sliding_window.rs:466-475 keeps map_points as
// [f32; 3]); 32 B, 4 per 128-B line
struct alignas(32) PnpEntry {
    uint64_t id;
    float pw[3];
    uint32_t pad;
};
static_assert(sizeof(PnpEntry) == 32, "4 entries per 128-B bucket");

__host__ __device__ __forceinline__ uint32_t map_bucket(uint64_t id, int mask) {
    return (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> 40) & (uint32_t)mask;  // Fibonacci hashing
}

enum { LM_COST_TOL = 1, LM_PARAM_TOL = 2, LM_MAX_ITERS = 3, LM_TRUST_REGION = 4, LM_NUMFAIL = -1, LM_SKIPPED = -2,
       LM_LINSOLVE = -3 };

struct PnpArgs {
    const uint8_t* ids[2];   // u64 feature ids, `id_stride` bytes apart
    int id_stride;
    const float2* uv[2];     // undistorted coordinates (frame.rs:118-119,131-132)
    const int* dcount;       // device (n_l, n_r), or null: n[] below
    int n[2];
    const PnpEntry* table;   // the map as a bucketed hash table (MapTable)
    int bucket_mask;         // buckets - 1 (a power of two)
    int max_probe;           // the longest bucket run an insertion took (lookups stop there)
    int has_top;             // a map point has the id kEmptyId (not representable in the table)
    float top_pw[3];         // ... its p_W
    int n_map;
    double T_last[16];
    double q0[4];            // from_matrix(R_B_W) of the last keyframe (host, rotation.hpp)
    double TCB[2][16];
    int max_iter;
    double cost_tol, param_tol, huber_delta, lambda0, thr_t, thr_r;
    rsvio_motion_result* out;  // pinned host memory
    double wclk_khz;           // device wall clock rate (kernel_ms)
};

// LM control state: wave 0's registers, every lane holding the same values
struct Ctl {
    double x[7], xt[7], H[21], g[6];
    double R[9], Rt[9];       // R_BW of x and of xt (pose_from7), cached for SE3 (+) and the pass
    double cost, lambda, nu, initial_cost, pred;
    int it, status, phase, run, n_obs;
};

__device__ __forceinline__ int utri6(int a, int c) { return a * 6 - (a * (a - 1)) / 2 + (c - a); }

// 64-bit cross-lane moves built from 32-bit lane ops
__device__ __forceinline__ void swap32_f64(double& x, double& y) {  // v_permlane32_swap
    const auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(x), __double2loint(y), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(x), __double2hiint(y), false, false);
    x = __hiloint2double(hi[0], lo[0]);
    y = __hiloint2double(hi[1], lo[1]);
}
__device__ __forceinline__ void swap16_f64(double& x, double& y) {  // v_permlane16_swap
    const auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(x), __double2loint(y), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(x), __double2hiint(y), false, false);
    x = __hiloint2double(hi[0], lo[0]);
    y = __hiloint2double(hi[1], lo[1]);
}

// Deterministic reduce-scatter of 32 per-lane values over the wave: afterwards lanes 2p and
// 2p+1 hold the wave total of value p.  Pairings (fixed, so results are run-to-run
// identical): lanes l / l+32 (permlane32 swap), rows 0/1 and 2/3 (permlane16 swap), then
// inside each row l / l^8 (row_ror 8), the half-row mirror, quad xor 2, quad xor 1.  About
// 125 instructions instead of 32 separate wave sums (~700).
__device__ __forceinline__ double wave_reduce_scatter32(double (&v)[32], int lane) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        swap32_f64(v[i], v[16 + i]);
        v[i] = v[i] + v[16 + i];   // lanes 0-31: value i, lanes 32-63: value 16+i
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        swap16_f64(v[i], v[8 + i]);
        v[i] = v[i] + v[8 + i];    // row r: value 8r' + i (r' = row parity within the half)
    }
    const bool b3 = lane & 8, b2 = lane & 4, b1 = lane & 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double keep = b3 ? v[4 + i] : v[i], send = b3 ? v[i] : v[4 + i];
        v[i] = keep + dpp64<0x128>(send);    // row_ror:8 -> lane l^8
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double keep = b2 ? v[2 + i] : v[i], send = b2 ? v[i] : v[2 + i];
        v[i] = keep + dpp64<0x141>(send);    // row_half_mirror: l <-> 7-l in each half-row
    }
    {
        const double keep = b1 ? v[1] : v[0], send = b1 ? v[0] : v[1];
        v[0] = keep + dpp64<0x4E>(send);     // quad_perm [2,3,0,1]
    }
    return v[0] + dpp64<0xB1>(v[0]);         // quad_perm [1,0,3,2]
}

// PnPFactor::linearize restated in T_C_W = T_C_B T_B_W (computed once per pass): p_C = R p_W + t,
// r = (x/z, y/z) - obs, dr/dt = jac_proj R_CW, dr/dw = jac_proj R_CB (-R_BW [p_W]x) = -(dr/dt) [p_W]x,
// i.e. row i of dr/dw is -(row i of dr/dt) x p_W.  Same values as factors.rs:545-571 up to
// rounding (~60 flops instead of ~180; 1/z by the refined hardware reciprocal; tolerance parity
// with the oracle's reference order).
__device__ __forceinline__ void pnp_linearize_cw(const double pW[3], const double uv[2], const double* T,
                                                 double r[2], double J[2][6]) {
    const double pC0 = ((T[0] * pW[0] + T[1] * pW[1]) + T[2] * pW[2]) + T[9];
    const double pC1 = ((T[3] * pW[0] + T[4] * pW[1]) + T[5] * pW[2]) + T[10];
    const double pC2 = ((T[6] * pW[0] + T[7] * pW[1]) + T[8] * pW[2]) + T[11];
    const double iz = rcp_f64(pC2);
    const double x = pC0 * iz, y = pC1 * iz;
    r[0] = x - uv[0];
    r[1] = y - uv[1];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        J[0][j] = iz * (T[j] - x * T[6 + j]);
        J[1][j] = iz * (T[3 + j] - y * T[6 + j]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        J[i][3] = J[i][2] * pW[1] - J[i][1] * pW[2];
        J[i][4] = J[i][0] * pW[2] - J[i][2] * pW[0];
        J[i][5] = J[i][1] * pW[0] - J[i][0] * pW[1];
    }
}

// Huber(delta) (factors.rs, the Ceres-style rho and IRLS weight as se3.hpp's huber) with one
// refined reciprocal square root instead of sqrt + a division: rho = 2 d s / sqrt(s) - d^2,
// w = d / sqrt(s) (tolerance parity)
__device__ __forceinline__ void pnp_huber(double s, double d, double* rho, double* w) {
    const double d2 = d * d;
    if (s <= d2) {
        *rho = s;
        *w = 1.0;
    } else {
        const double is = rsqrt_f64(s);
        *rho = 2.0 * d * (s * is) - d2;
        *w = d * is;
    }
}

// (H + lambda I) dx = -g by LDL^T with hardware-reciprocal pivots (no square root, no IEEE
// division on the serial chain).  Positive definiteness is tested on the pivots exactly like
// the oracle's Cholesky (chol_solve) tests d > 0; the solution agrees to rounding (tolerance
// parity).  All operands in registers (wave 0, every lane the same values).
__device__ __forceinline__ bool ldl6(const double (&Hp)[21], double lambda, const double (&g)[6], double (&dx)[6]) {
    double A[6][6];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = a; c < 6; ++c) A[c][a] = Hp[utri6(a, c)];  // lower triangle
#pragma unroll
    for (int a = 0; a < 6; ++a) A[a][a] += lambda;
    double L[6][6], U[6][6], inv[6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * U[j][k];
        ok &= (d > 0.0) && isfinite(d);
        inv[j] = rcp_f64(d);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double u = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) u -= L[i][k] * U[j][k];
            U[i][j] = u;
            L[i][j] = u * inv[j];
        }
    }
    double z[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = -g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i][k] * z[k];
        z[i] = s;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = z[i] * inv[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s -= L[k][i] * dx[k];
        dx[i] = s;
    }
    return ok;
}

__device__ __forceinline__ void rot_from_unit_quat(const double* q, double* R) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    const double xy = x * y * 2.0, wz = w * z * 2.0, wy = w * y * 2.0;
    const double xz = x * z * 2.0, yz = y * z * 2.0, wx = w * x * 2.0;
    R[0] = ww + xx - yy - zz; R[1] = xy - wz;           R[2] = wy + xz;
    R[3] = wz + xy;           R[4] = ww - xx + yy - zz; R[5] = yz - wx;
    R[6] = xz - wy;           R[7] = wx + yz;           R[8] = ww - xx - yy + zz;
}

// se3_plus with the rotation of x7 given (cached) and the rotation of the result returned
// (from its normalised quaternion).  The four functions of theta by se3.hpp's power series in
// theta^2 for |theta| < 1/4 (an LM step's rotation: no square root, sincos or division on the
// chain), one sincos of theta / 2 otherwise -- the BA's se3_plus; tolerance parity.
__device__ __forceinline__ void se3_plus_r(const double (&p7)[7], const double (&R)[9], const double (&d)[6],
                                           double (&out)[7], double (&Rout)[9]) {
    const double* rho = d;
    const double* om = d + 3;
    const double th2 = om[0] * om[0] + om[1] * om[1] + om[2] * om[2];
    double qd[4], Ac, Bc;
    if (th2 < 0.0625) {
        const double s = se3_series<1>(th2);  // sin(theta/2) / theta
        qd[0] = se3_series<0>(th2);           // cos(theta/2)
        qd[1] = s * om[0]; qd[2] = s * om[1]; qd[3] = s * om[2];
        Ac = se3_series<2>(th2);
        Bc = se3_series<3>(th2);
    } else {
        const double th = sqrt(th2);
        double sh, ch;
        sincos(0.5 * th, &sh, &ch);
        const double ith = rcp_f64(th);
        const double sth = sh * ith;
        qd[0] = ch; qd[1] = sth * om[0]; qd[2] = sth * om[1]; qd[3] = sth * om[2];
        const double ith2 = ith * ith;
        Ac = 2.0 * sh * sh * ith2;
        Bc = (th - 2.0 * sh * ch) * ith2 * ith;
    }
    const double wx[3] = {om[1] * rho[2] - om[2] * rho[1], om[2] * rho[0] - om[0] * rho[2],
                          om[0] * rho[1] - om[1] * rho[0]};
    const double wwx[3] = {om[1] * wx[2] - om[2] * wx[1], om[2] * wx[0] - om[0] * wx[2],
                           om[0] * wx[1] - om[1] * wx[0]};
    double td[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) td[i] = rho[i] + Ac * wx[i] + Bc * wwx[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = p7[i] + ((R[3 * i] * td[0] + R[3 * i + 1] * td[1]) + R[3 * i + 2] * td[2]);
    const double w0 = p7[3], x0 = p7[4], y0 = p7[5], z0 = p7[6];
    double qn[4] = {w0 * qd[0] - x0 * qd[1] - y0 * qd[2] - z0 * qd[3], w0 * qd[1] + x0 * qd[0] + y0 * qd[3] - z0 * qd[2],
                    w0 * qd[2] - x0 * qd[3] + y0 * qd[0] + z0 * qd[1], w0 * qd[3] + x0 * qd[2] - y0 * qd[1] + z0 * qd[0]};
    const double inn = rsqrt_f64(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[3 + i] = qn[i] * inn;
    rot_from_unit_quat(out + 3, Rout);
}

// Lane 0 of wave 0 between passes (the state in LDS: its registers are the pass's): consume the
// pass sums, then either set up the next pass at a trial pose (C.run = 1, its R_BW and t_BW in
// pose[12]) or finish (run = 0).  Mirrors oracle orc_track_motion's loop step for step.
__device__ __forceinline__ void pnp_control(const PnpArgs& A, Ctl& C, const double* __restrict__ sum,
                                         double* __restrict__ pose) {
    bool done = false;
    if (C.phase == 0) {
#pragma unroll
        for (int k = 0; k < 21; ++k) C.H[k] = sum[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) C.g[k] = sum[21 + k];
        C.cost = sum[27];
        C.initial_cost = C.cost;
        C.phase = 1;
    } else {
        const double new_cost = sum[27];
        const double dcost = C.cost - new_cost;
        const double rho = dcost / C.pred;
        if (isfinite(new_cost) && fabs(dcost) <= A.cost_tol * C.cost) {
            // converged: the change is within the tolerance whatever its sign, the candidate not
            // applied (the BA's lm_update takes the same decision).  This
            // build's rule, a deliberate departure: apex-solver's is absent offline (unpinned)
            C.status = LM_COST_TOL;
            done = true;
        } else if (isfinite(new_cost) && rho > 0.0) {
#pragma unroll
            for (int k = 0; k < 7; ++k) C.x[k] = C.xt[k];
#pragma unroll
            for (int k = 0; k < 9; ++k) C.R[k] = C.Rt[k];
#pragma unroll
            for (int k = 0; k < 21; ++k) C.H[k] = sum[k];
#pragma unroll
            for (int k = 0; k < 6; ++k) C.g[k] = sum[21 + k];
            const double f = 2.0 * rho - 1.0;
            C.lambda *= fmax(1.0 / 3.0, 1.0 - f * f * f);
            C.nu = 2.0;
            C.cost = new_cost;
        } else {
            C.lambda *= C.nu;
            C.nu *= 2.0;
            if (C.lambda > 1e32) {
                C.status = LM_TRUST_REGION;
                done = true;
            }
        }
    }
    C.run = 0;
    if (done) return;
    if (C.it >= A.max_iter) {
        C.status = LM_MAX_ITERS;
        return;
    }
    C.it += 1;
    if (!isfinite(C.cost)) {
        C.status = LM_NUMFAIL;
        return;
    }
    double dx[6], H[21], g[6];
#pragma unroll
    for (int k = 0; k < 21; ++k) H[k] = C.H[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = C.g[k];
    const bool solved = ldl6(H, C.lambda, g, dx);
    STAMP(30);
    if (!solved) {  // Err(LinearSolveFailed) -> track_motion returns Ok(None) (:554-560)
        C.status = LM_LINSOLVE;
        return;
    }
    double dx2 = 0.0, gdx = 0.0, x2 = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        dx2 += dx[k] * dx[k];
        gdx += g[k] * dx[k];
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) x2 += C.x[k] * C.x[k];
    if (sqrt(dx2) <= A.param_tol * (sqrt(x2) + A.param_tol)) {
        C.status = LM_PARAM_TOL;
        return;
    }
    double x[7], R[9], xt[7], Rt[9];
#pragma unroll
    for (int k = 0; k < 7; ++k) x[k] = C.x[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = C.R[k];
    se3_plus_r(x, R, dx, xt, Rt);
#pragma unroll
    for (int k = 0; k < 7; ++k) C.xt[k] = xt[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) C.Rt[k] = Rt[k];
    STAMP(31);
    C.pred = 0.5 * (C.lambda * dx2 - gdx);
#pragma unroll
    for (int k = 0; k < 9; ++k) pose[k] = Rt[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) pose[9 + k] = xt[k];
    C.run = 1;
}

// lane 0 of wave 0
__device__ void pnp_finish(const PnpArgs& A, const Ctl& C, unsigned long long t_entry) {
    rsvio_motion_result r;
    r.status = C.status;
    r.iterations = C.it;
    r.n_observations = C.n_obs;
    r.initial_cost = C.initial_cost;
    r.final_cost = C.cost;
    r.translation_norm = 0.0;
    r.rotation_norm = 0.0;
    const bool ok = C.status > 0;
    if (ok) {
        // T_W_B = inv(SE3(F).matrix()) (sliding_window.rs:566-569)
        const Pose P = pose_from7(C.x);
        double TBW[16];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) TBW[4 * i + j] = P.R[i][j];
            TBW[4 * i + 3] = P.t[i];
        }
        TBW[12] = 0.0; TBW[13] = 0.0; TBW[14] = 0.0; TBW[15] = 1.0;
        rigid_inverse(TBW, r.T_W_B);
        // the keyframe rule (estimator.rs:204-225) runs on the host after the kernel
        // (keyframe_rule(): nalgebra's iterative from_matrix is a long serial loop)
        r.is_keyframe = 0;
    } else {
        for (int k = 0; k < 16; ++k) r.T_W_B[k] = (k % 5 == 0) ? 1.0 : 0.0;
        r.is_keyframe = 1;
    }
    r.kernel_ms = (double)(wall_clock64() - t_entry) / A.wclk_khz;
    *A.out = r;
}

// The map point of `id` (map_points.get, sliding_window.rs:526-545): the bucket of its hash, then
// the following ones up to the longest run an insertion took; a bucket with a free entry ends a
// miss.  One 128-B load per bucket visited (almost always one).
__device__ __forceinline__ bool map_lookup(const PnpArgs& A, uint64_t id, float (&pw)[3]) {
    if (id == kEmptyId) {
        pw[0] = A.top_pw[0]; pw[1] = A.top_pw[1]; pw[2] = A.top_pw[2];
        return A.has_top != 0;
    }
    uint32_t b = map_bucket(id, A.bucket_mask);
    for (int p = 0; p <= A.max_probe; ++p) {
        // the bucket's 4 entries as 8 16-B loads, all in flight; the match picked by selects (no
        // runtime-indexed local array: that would go through scratch)
        const uint4* e = reinterpret_cast<const uint4*>(A.table + (size_t)b * kBucket);
        uint4 v[2 * kBucket];
#pragma unroll
        for (int k = 0; k < 2 * kBucket; ++k) v[k] = e[k];
        bool hit = false, free_slot = false;
        uint32_t x = 0, y = 0, z = 0;
#pragma unroll
        for (int k = 0; k < kBucket; ++k) {
            const uint64_t key = (uint64_t)v[2 * k].x | ((uint64_t)v[2 * k].y << 32);
            const bool m = key == id;
            x = m ? v[2 * k].z : x;
            y = m ? v[2 * k].w : y;
            z = m ? v[2 * k + 1].x : z;
            hit |= m;
            free_slot |= key == kEmptyId;
        }
        if (hit) {
            pw[0] = __uint_as_float(x); pw[1] = __uint_as_float(y); pw[2] = __uint_as_float(z);
            return true;
        }
        if (free_slot) return false;
        b = (b + 1) & (uint32_t)A.bucket_mask;
    }
    return false;
}

// ---- the LM both bodies run (pnp_track_motion_body here, pnp_robust_refit_body in pnp_robust.hpp) ----

// The LDS of one LM: the factor list (feature j at entry j), the pass sums and the LM state.  Each
// body declares one __shared__ instance; CAP: the entries for features.  16-byte aligned, and so
// every array and the state in it (the alignment separate __shared__ variables get: 16-byte LDS
// accesses); the two ints last, so nothing is padded.
template <int CAP>
struct alignas(16) LmLds {
    float s_mpw[3][CAP];              // the map point per factor
    float s_uv[2][CAP];               // undistorted coordinates per factor
    int8_t s_cam[CAP];                // feature -> camera, -1: no factor
    double s_red[kPnpWaves][kRed];
    double s_sum[kRed];
    double s_pose[12];                // R_BW, t_BW of the pass pose (wave 0's)
    double s_tcb[2][16];
    double s_tcw[2][12];              // T_C_W = T_C_B T_B_W per camera at the pass pose
    Ctl s_ctl;                        // the LM state between controls (wave 0's)
    int s_nobs;                       // the factors
    int s_run;
};
static_assert(offsetof(LmLds<kPnpMaxFeatures>, s_ctl) % 16 == 0, "the LM state in 16-byte LDS accesses");

// Entry e of T_C_W = T_C_B [R | t] as 12 values (R row-major, then t); T: one camera's T_C_B (16),
// pose: R (9), t (3)
__device__ __forceinline__ double tcw_entry(const double* T, const double* pose, int e) {
    if (e < 9) {
        const int i = e / 3, j = e % 3;
        return (T[4 * i] * pose[j] + T[4 * i + 1] * pose[3 + j]) + T[4 * i + 2] * pose[6 + j];
    }
    const int i = e - 9;
    return ((T[4 * i] * pose[9] + T[4 * i + 1] * pose[10]) + T[4 * i + 2] * pose[11]) + T[4 * i + 3];
}

// The pose7 the LM starts from at the last keyframe, T_B_W = inv(T_W_B) with the host's
// q = UnitQuaternion::from_matrix(R_B_W) (sliding_window.rs:506-517), and its rotation by SE3::from
// (apex) of that 7-vector
__device__ __forceinline__ void prior_pose(const PnpArgs& A, double x[7], double R[9]) {
    double TBW[16];
    rigid_inverse(A.T_last, TBW);
    x[0] = TBW[3];
    x[1] = TBW[7];
    x[2] = TBW[11];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[3 + k] = A.q0[k];
    const Pose P0 = pose_from7(x);
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = P0.R[k / 3][k % 3];
}

// The LM state before its first pass, all but the pose (x, R)
__device__ __forceinline__ void ctl_start(const PnpArgs& A, Ctl& C) {
    C.it = 0;
    C.status = LM_MAX_ITERS;
    C.phase = 0;
    C.lambda = A.lambda0;
    C.nu = 2.0;
    C.cost = 0.0;
    C.initial_cost = 0.0;
    C.pred = 0.0;
}

// Lane 0 of wave 0: the start pose as the first pass's, and the state to LDS
__device__ __forceinline__ void ctl_publish(const Ctl& C, double* s_pose, Ctl& s_ctl) {
#pragma unroll
    for (int k = 0; k < 9; ++k) s_pose[k] = C.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s_pose[9 + k] = C.x[k];
    s_ctl = C;
}

// The pass loop: while `run`, one pass at the pose in s_tcw (H, g and the cost over the factors
// of S, lane t taking entries t, t + 512, ... of the nf features; DPP reduce-scatter per wave, then
// the waves in order), lane 0's pnp_control, and the next pass's T_C_W by wave 0.  Two workgroup
// barriers per pass.  STAMPS: the plain kernel's stamp points 3..26 (two per pass, 12 passes).
template <bool STAMPS, int CAP>
__device__ __forceinline__ void lm_passes(const PnpArgs& A, LmLds<CAP>& S, int nf, int run) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int pass = 0;
    while (run) {
        if (STAMPS && pass < 12) STAMP(3 + 2 * pass);
        // one pass at the pose in s_tcw: H, g, cost over this lane's observations (j order)
        double acc[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) acc[k] = 0.0;
#pragma unroll 1
        for (int j = tid; j < nf; j += kPnpThreads) {
            const int cam = S.s_cam[j];
            if (cam < 0) continue;
            const double pW[3] = {(double)S.s_mpw[0][j], (double)S.s_mpw[1][j], (double)S.s_mpw[2][j]};
            const double uv[2] = {(double)S.s_uv[0][j], (double)S.s_uv[1][j]};
            double r[2], J[2][6];
            pnp_linearize_cw(pW, uv, S.s_tcw[cam], r, J);
            const double s2 = r[0] * r[0] + r[1] * r[1];
            double rho, w;
            pnp_huber(s2, A.huber_delta, &rho, &w);
            acc[27] += 0.5 * rho;
            const double wr0 = w * r[0], wr1 = w * r[1];
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double w0 = w * J[0][a], w1 = w * J[1][a];
#pragma unroll
                for (int c = a; c < 6; ++c) acc[utri6(a, c)] += w0 * J[0][c] + w1 * J[1][c];
                acc[21 + a] += J[0][a] * wr0 + J[1][a] * wr1;
            }
        }
        {
            const double v = wave_reduce_scatter32(acc, lane);
            if ((lane & 1) == 0 && (lane >> 1) < kRed) S.s_red[wv][lane >> 1] = v;
        }
        __syncthreads();  // every wave's partials
        if (STAMPS && pass < 12) STAMP(4 + 2 * pass);
        ++pass;
        if (wv == 0) {
            // the waves in order (lane k sums value k), then lane 0's control
            if (lane < kRed) {
                double v = S.s_red[0][lane];
#pragma unroll
                for (int w = 1; w < kPnpWaves; ++w) v += S.s_red[w][lane];
                S.s_sum[lane] = v;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) {
                pnp_control(A, S.s_ctl, S.s_sum, S.s_pose);
                S.s_run = S.s_ctl.run;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (S.s_run && lane < 24) {
                const int c = lane / 12, e = lane % 12;
                S.s_tcw[c][e] = tcw_entry(S.s_tcb[c], S.s_pose, e);
            }
        }
        __syncthreads();  // s_run and the next pass's T_C_W
        run = S.s_run;
    }
}

// The whole of track_motion for one frame, run by one workgroup of kPnpThreads lanes: the body of
// pnp_track_motion_kernel (A by value, in the kernel arguments) and of
// pnp_track_motion_batch_kernel (A in a device table, one entry per workgroup).  CAP: the LDS
// entries for features (feature j at entry j whatever CAP is, so CAP changes no result).
template <int CAP>
__device__ __forceinline__ void pnp_track_motion_body(const PnpArgs& A) {
    __shared__ LmLds<CAP> S;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    STAMP(0);
    const unsigned long long t_entry = wall_clock64();  // (kept by thread 0 for kernel_ms)
    const int n0 = A.dcount ? A.dcount[0] : A.n[0];
    const int n1 = A.dcount ? A.dcount[1] : A.n[1];
    const int nf = n0 + n1;
    const bool fits = nf <= CAP;
    // the factor list: features with a map point, left then right (sliding_window.rs:519-547);
    // feature j's observation goes to LDS entry j (cam -1: no map point).  Two features per lane
    // per round: both id / uv loads, then both bucket loads in flight together.
    int mine = 0;
    if (tid == 0) S.s_nobs = 0;
    if (tid < 32) S.s_tcb[tid >> 4][tid & 15] = A.TCB[tid >> 4][tid & 15];
    for (int j0 = tid; j0 < nf && fits; j0 += 2 * kPnpThreads) {
        uint64_t id[2];
        float2 q[2];
        int cam[2];
        bool v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = j0 + h * kPnpThreads;
            v[h] = j < nf;
            const int jj = v[h] ? j : j0;
            cam[h] = jj < n0 ? 0 : 1;
            const int i = cam[h] == 0 ? jj : jj - n0;
            id[h] = *reinterpret_cast<const uint64_t*>(A.ids[cam[h]] + (size_t)i * A.id_stride);
            q[h] = A.uv[cam[h]][i];
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (!v[h]) continue;
            const int j = j0 + h * kPnpThreads;
            float pw[3];
            const bool hit = A.n_map > 0 && map_lookup(A, id[h], pw);
            S.s_cam[j] = hit ? (int8_t)cam[h] : (int8_t)-1;
            if (hit) {
                S.s_uv[0][j] = q[h].x;
                S.s_uv[1][j] = q[h].y;
                S.s_mpw[0][j] = pw[0];
                S.s_mpw[1][j] = pw[1];
                S.s_mpw[2][j] = pw[2];
                ++mine;
            }
        }
    }
    // wave 0: the LM state (LDS between controls, registers during one); F starts from the last
    // keyframe (sliding_window.rs:506-517)
    if (wv == 0) {
        Ctl C;
        ctl_start(A, C);
        prior_pose(A, C.x, C.R);
        if (lane == 0) ctl_publish(C, S.s_pose, S.s_ctl);
    }
    // per-wave total (one LDS atomic per wave instead of one per lane)
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    __syncthreads();  // s_nobs = 0, s_tcb and s_pose (wave 0) before their uses
    if (lane == 0 && mine) atomicAdd(&S.s_nobs, mine);
    if (wv == 0) {
        if (lane < 24) {  // T_C_W = T_C_B T_B_W, one entry per lane
            const int c = lane / 12, e = lane % 12;
            S.s_tcw[c][e] = tcw_entry(S.s_tcb[c], S.s_pose, e);
        }
    }
    STAMP(1);
    __syncthreads();  // the factor list, s_nobs and the first T_C_W
    STAMP(2);
    const int nobs = S.s_nobs;
    const int run = (fits && nobs > 0) ? 1 : 0;
    if (tid == 0) {
        S.s_ctl.n_obs = fits ? nobs : -1;
        if (!run) S.s_ctl.status = LM_SKIPPED;  // no factor: treated as a failed optimisation
    }
    lm_passes<true>(A, S, nf, run);
    STAMP(28);
    if (tid == 0) pnp_finish(A, S.s_ctl, t_entry);
    STAMP(29);
}

__global__ __launch_bounds__(kPnpThreads) void pnp_track_motion_kernel(PnpArgs A) {
    pnp_track_motion_body<kPnpMaxFeatures>(A);
}

// Batched: workgroup blockIdx.x is stream i, its arguments entry i of a table in device memory
// (uniform over the workgroup: scalar loads).  No workgroup reads what another writes.
template <int CAP>
__global__ __launch_bounds__(kPnpThreads) void pnp_track_motion_batch_kernel(const PnpArgs* __restrict__ table) {
    pnp_track_motion_body<CAP>(table[blockIdx.x]);
}

#include "pnp_robust.hpp"
#include "pnp_covariance.hpp"

}  // namespace

RSVIO_DBG_READER(rsvio_dbg_pnp_stamps)

struct Pnp {
    int device = 0;
    hipStream_t stream = nullptr;      // the handle's own
    hipStream_t user = nullptr;        // rsvio_pnp_set_stream
    hipStream_t active() const { return user ? user : stream; }
    // the map as a bucketed hash table (set_map): kBucket entries per bucket, a power of two of
    // buckets with at most one entry per kBucket slots used (load <= 1/4)
    DevBuf<PnpEntry> table;
    std::vector<PnpEntry> htable;
    int bucket_mask = 0, max_probe = 0, has_top = 0;
    float top_pw[3] = {0.f, 0.f, 0.f};
    int n_map = 0;
    DevBuf<uint8_t> feat;            // [ids_l | ids_r | uv_l | uv_r]
    HostBuf<uint8_t> hfeat;
    HostBuf<rsvio_motion_result> hres;
    double wclk_khz = 1.0e5;
    double q0_key[16] = {};              // T_W_B_last_kf of the cached initial quaternion
    double q0[4] = {1.0, 0.0, 0.0, 0.0};
    // the robust path's scratch (pnp_robust.hpp), allocated by its first call
    DevBuf<double> rdbl;                 // w, uv, pair_q, pair_w, hyp_pose
    DevBuf<int> rint;                    // cam, pos, pair_ok, counts, hyp_count, samples
    DevBuf<uint8_t> rmask;
    HostBuf<rsvio_robust_motion_result> hrobust;
    HostBuf<int> hrint;                  // samples (staging), hyp_count (read back)
    HostBuf<uint8_t> hrmask;
    hipEvent_t rev[2] = {nullptr, nullptr};
    // the covariance call's (pnp_covariance.hpp), allocated by its first call
    HostBuf<CovOut> hcov;
    DevBuf<uint8_t> cmask;               // [mask_l | mask_r]
    HostBuf<uint8_t> hcmask;

    void init_cov() {
        if (hcov.p) return;
        cmask.alloc(kPnpMaxFeatures);
        hcmask.alloc(kPnpMaxFeatures);
        hcov.alloc(1);
    }

    void init_robust() {
        if (rev[1]) return;
        rdbl.alloc(kRobustDbl);
        rint.alloc(kRobustInt + 4 * kRansacMaxHyp);  // ... hyp_count, samples (3 per hypothesis)
        rmask.alloc(kPnpMaxFeatures);
        hrobust.alloc(1);
        hrint.alloc(4 * kRansacMaxHyp);
        hrmask.alloc(kPnpMaxFeatures);
        RSVIO_HIP(hipEventCreate(&rev[0]));
        RSVIO_HIP(hipEventCreate(&rev[1]));
    }

    void init(int dev) {
        device = dev;
        RSVIO_HIP(hipSetDevice(dev));
        RSVIO_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        hres.alloc(1);
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && khz > 0)
            wclk_khz = khz;
        (void)hipGetLastError();
    }
    ~Pnp() {
        for (hipEvent_t e : rev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

PnpArgs make_args(Pnp& p, const double* T_last, const double* TCB2, const rsvio_lm_cfg* cfg,
                  const rsvio_keyframe_rule* rule) {
    PnpArgs A{};
    A.table = p.table.p;
    A.bucket_mask = p.bucket_mask;
    A.max_probe = p.max_probe;
    A.has_top = p.has_top;
    for (int k = 0; k < 3; ++k) A.top_pw[k] = p.top_pw[k];
    A.n_map = p.n_map;
    std::memcpy(A.T_last, T_last, sizeof(A.T_last));
    std::memcpy(A.TCB, TCB2, sizeof(A.TCB));
    A.max_iter = cfg->max_iterations;
    A.cost_tol = cfg->cost_tolerance;
    A.param_tol = cfg->parameter_tolerance;
    A.huber_delta = cfg->huber_delta;
    A.lambda0 = cfg->lambda_init;
    A.thr_t = rule->translation_threshold;
    A.thr_r = rule->rotation_threshold;
    A.out = p.hres.p;
    A.wclk_khz = p.wclk_khz;
    // sliding_window.rs:506-517: F starts from the last keyframe's T_B_W = inv(T_W_B) with
    // q = UnitQuaternion::from_matrix(R_B_W); cached per keyframe pose
    if (std::memcmp(p.q0_key, T_last, sizeof p.q0_key) != 0) {
        double TBW[16];
        rigid_inverse(T_last, TBW);
        const double R[9] = {TBW[0], TBW[1], TBW[2], TBW[4], TBW[5], TBW[6], TBW[8], TBW[9], TBW[10]};
        rot::quat_from_matrix(R, p.q0);
        std::memcpy(p.q0_key, T_last, sizeof p.q0_key);
    }
    std::memcpy(A.q0, p.q0, sizeof A.q0);
    return A;
}

// The keyframe rule (estimator.rs:204-225) on the PnP result: T_rel = T_W_B inv(T_W_B_last_kf),
// keyframe iff |t_rel| > thr_t or |euler(from_matrix(R_rel))| > thr_r.  A failed PnP keeps
// is_keyframe = 1 and T_W_B = I (written by the kernel, estimator.rs:228-234).
void keyframe_rule(const PnpArgs& A, rsvio_motion_result* r) {
    if (r->status <= 0) return;
    double Tl_inv[16], Tr[16];
    rigid_inverse(A.T_last, Tl_inv);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += r->T_W_B[4 * i + k] * Tl_inv[4 * k + j];
            Tr[4 * i + j] = s;
        }
    r->translation_norm = std::sqrt((Tr[3] * Tr[3] + Tr[7] * Tr[7]) + Tr[11] * Tr[11]);
    const double Rr[9] = {Tr[0], Tr[1], Tr[2], Tr[4], Tr[5], Tr[6], Tr[8], Tr[9], Tr[10]};
    double q[4], Q[9];
    rot::quat_from_matrix(Rr, q);
    rot::rotation_of_quat(q, Q);
    r->rotation_norm = rot::euler_norm(Q);
    r->is_keyframe = (r->translation_norm > A.thr_t || r->rotation_norm > A.thr_r) ? 1 : 0;
}

int run_pnp(Pnp& p, const PnpArgs& A, hipStream_t stream, rsvio_motion_result* res) {
    hipLaunchKernelGGL(pnp_track_motion_kernel, dim3(1), dim3(kPnpThreads), 0, stream, A);
    RSVIO_HIP(hipGetLastError());
    RSVIO_HIP(hipStreamSynchronize(stream));
    *res = *p.hres.p;
    keyframe_rule(A, res);
    if (res->n_observations < 0) {
        set_last_error("track_motion: more than 4096 features in one frame");
        return RSVIO_ERR_CAPACITY;
    }
    return RSVIO_OK;
}

// A staged frame: [ids_l | ids_r | uv_l | uv_r] at `base`, 8 bytes per id and per coordinate pair,
// 16 (n_l + n_r) in all.  pack_frame writes it from host arrays, packed_lists points A's lists at it.
void pack_frame(uint8_t* base, const uint64_t* ids_l, const float* uv_l, size_t n_l, const uint64_t* ids_r,
                const float* uv_r, size_t n_r) {
    const size_t n = n_l + n_r;
    if (n_l) std::memcpy(base, ids_l, 8 * n_l);
    if (n_r) std::memcpy(base + 8 * n_l, ids_r, 8 * n_r);
    if (n_l) std::memcpy(base + 8 * n, uv_l, 8 * n_l);
    if (n_r) std::memcpy(base + 8 * n + 8 * n_l, uv_r, 8 * n_r);
}

void packed_lists(const uint8_t* base, size_t n_l, size_t n_r, PnpArgs& A) {
    const size_t n = n_l + n_r;
    A.ids[0] = base;
    A.ids[1] = base + 8 * n_l;
    A.id_stride = 8;
    A.uv[0] = reinterpret_cast<const float2*>(base + 8 * n);
    A.uv[1] = reinterpret_cast<const float2*>(base + 8 * n + 8 * n_l);
    A.dcount = nullptr;
    A.n[0] = (int)n_l;
    A.n[1] = (int)n_r;
}

// A frame given as host arrays: staged and uploaded on the handle's stream, A's lists set to it
void host_frame(Pnp& P, const uint64_t* ids_l, const float* uv_l, size_t n_l, const uint64_t* ids_r,
                const float* uv_r, size_t n_r, PnpArgs& A) {
    const size_t bytes = (n_l + n_r) * 16;
    if (P.feat.n < bytes || !P.feat.p) {
        const size_t cap = (size_t)kPnpMaxFeatures * 16;
        P.feat.alloc(cap);
        P.hfeat.alloc(cap);
    }
    pack_frame(P.hfeat.p, ids_l, uv_l, n_l, ids_r, uv_r, n_r);
    if (bytes) RSVIO_HIP(hipMemcpyAsync(P.feat.p, P.hfeat.p, bytes, hipMemcpyHostToDevice, P.active()));
    packed_lists(P.feat.p, n_l, n_r, A);
}

// The tracker's last collected frame, read in place: A's lists set to its output slot
int tracker_frame(Pnp& P, rsvio_tracker* t, PnpArgs& A) {
    const TrackerView v = tracker_view(t);
    if (!v.undist[0]) {
        set_last_error("rsvio_track_motion_tracker: attach cameras to the tracker first");
        return (int)RSVIO_ERR_INVALID_ARG;
    }
    if (v.device != P.device) {
        set_last_error("rsvio_track_motion_tracker: tracker and pnp handle on different devices");
        return (int)RSVIO_ERR_INVALID_ARG;
    }
    RSVIO_HIP(hipSetDevice(P.device));
    if (v.n[0] + v.n[1] > kPnpMaxFeatures) {
        set_last_error("track_motion: more than 4096 features in one frame");
        return (int)RSVIO_ERR_CAPACITY;
    }
    // the map upload (set_map) is ordered before this launch: it synchronised its stream.  The
    // view is the last collected frame's output slot, complete on the device (its collect
    // waited for it), so the launch goes on the handle's own stream: it runs beside a next
    // frame already submitted to the tracker's stream, which writes the other slot
    A.ids[0] = reinterpret_cast<const uint8_t*>(v.out[0]);
    A.ids[1] = reinterpret_cast<const uint8_t*>(v.out[1]);
    A.id_stride = (int)sizeof(rsvio_feature);
    A.uv[0] = v.undist[0];
    A.uv[1] = v.undist[1];
    A.dcount = nullptr;
    A.n[0] = v.n[0];
    A.n[1] = v.n[1];
    return (int)RSVIO_OK;
}

bool ransac_cfg_ok(const rsvio_ransac_cfg* rc) {
    return rc && rc->n_hyp >= 1 && rc->n_hyp <= kRansacMaxHyp && rc->inlier_sq_error > 0.0;  // (NaN fails >)
}

// A timed section of `stream`: ev[0], what `launch` submits, ev[1], what `then` queues behind it
// (copies back, not timed), and the one host wait -> the milliseconds between the events
template <class Launch, class Then>
float timed_section(hipStream_t stream, hipEvent_t (&ev)[2], Launch launch, Then then) {
    RSVIO_HIP(hipEventRecord(ev[0], stream));
    launch();
    RSVIO_HIP(hipGetLastError());
    RSVIO_HIP(hipEventRecord(ev[1], stream));
    then();
    RSVIO_HIP(hipStreamSynchronize(stream));
    float ms = 0.f;
    RSVIO_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    return ms;
}

// The three launches of pnp_robust.hpp on `stream`, then the one host wait; A holds the feature
// lists (device pointers and counts, n_l + n_r <= kPnpMaxFeatures)
int run_pnp_robust(Pnp& p, PnpArgs A, hipStream_t stream, const rsvio_ransac_cfg* rc, const int32_t* samples,
                   uint8_t* mask_l, uint8_t* mask_r, int32_t* hyp_count, rsvio_robust_motion_result* res) {
    p.init_robust();
    const int n_l = A.n[0], n_r = A.n[1];
    RobustArgs RA{};
    A.out = &p.hrobust.p->motion;
    RA.P = A;
    RA.B = robust_carve(p.rdbl.p, p.rint.p);
    RA.B.hyp_count = p.rint.p + kRobustInt;
    int* d_samples = RA.B.hyp_count + kRansacMaxHyp;
    RA.B.mask = p.rmask.p;
    set_ransac(RA, rc);
    RA.out = p.hrobust.p;
    if (samples) {
        std::memcpy(p.hrint.p, samples, sizeof(int32_t) * 3 * (size_t)rc->n_hyp);
        RSVIO_HIP(hipMemcpyAsync(d_samples, p.hrint.p, sizeof(int32_t) * 3 * (size_t)rc->n_hyp, hipMemcpyHostToDevice,
                                 stream));
        RA.B.samples = d_samples;
    }
    int* h_counts = p.hrint.p + 3 * kRansacMaxHyp;
    const float ms = timed_section(
        stream, p.rev,
        [&] {
            hipLaunchKernelGGL(pnp_robust_join_kernel, dim3(1), dim3(kPnpThreads), 0, stream, RA);
            hipLaunchKernelGGL(pnp_robust_score_kernel, dim3(rc->n_hyp), dim3(64), 0, stream, RA);
            hipLaunchKernelGGL(pnp_robust_refit_kernel, dim3(1), dim3(kPnpThreads), 0, stream, RA);
        },
        [&] {
            if ((mask_l || mask_r) && n_l + n_r)
                RSVIO_HIP(hipMemcpyAsync(p.hrmask.p, p.rmask.p, (size_t)(n_l + n_r), hipMemcpyDeviceToHost, stream));
            if (hyp_count)
                RSVIO_HIP(hipMemcpyAsync(h_counts, RA.B.hyp_count, sizeof(int32_t) * (size_t)rc->n_hyp,
                                         hipMemcpyDeviceToHost, stream));
        });
    *res = *p.hrobust.p;
    keyframe_rule(A, &res->motion);
    res->device_ms = ms;
    if (mask_l && n_l) std::memcpy(mask_l, p.hrmask.p, (size_t)n_l);
    if (mask_r && n_r) std::memcpy(mask_r, p.hrmask.p + n_l, (size_t)n_r);
    if (hyp_count) std::memcpy(hyp_count, h_counts, sizeof(int32_t) * (size_t)rc->n_hyp);
    return RSVIO_OK;
}

// ---- motion covariance (pnp_covariance.hpp) ----

// The arguments of one covariance launch on handle p at T_W_B, lists not yet set: the map, and
// T_C_W = T_C_B inverse(T_W_B) per camera.  Touches nothing a tracking call reads (make_args
// caches the last keyframe's quaternion; this does not go through it).
CovArgs cov_args(const Pnp& p, const double* T_W_B, const double* TCB2, double huber_delta) {
    CovArgs A{};
    A.P.table = p.table.p;
    A.P.bucket_mask = p.bucket_mask;
    A.P.max_probe = p.max_probe;
    A.P.has_top = p.has_top;
    for (int k = 0; k < 3; ++k) A.P.top_pw[k] = p.top_pw[k];
    A.P.n_map = p.n_map;
    A.P.wclk_khz = p.wclk_khz;
    A.huber_delta = huber_delta;
    double TBW[16];
    rigid_inverse(T_W_B, TBW);
    for (int c = 0; c < 2; ++c) {
        const double* T = TCB2 + 16 * c;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j)
                A.TCW[c][3 * i + j] = (T[4 * i] * TBW[j] + T[4 * i + 1] * TBW[4 + j]) + T[4 * i + 2] * TBW[8 + j];
            A.TCW[c][9 + i] = ((T[4 * i] * TBW[3] + T[4 * i + 1] * TBW[7]) + T[4 * i + 2] * TBW[11]) + T[4 * i + 3];
        }
    }
    return A;
}

// One launch on `stream`, then the host wait; A.P holds the lists (device pointers and counts,
// n_l + n_r <= kPnpMaxFeatures), the masks are host arrays or null
int run_pnp_cov(Pnp& p, CovArgs A, hipStream_t stream, const uint8_t* mask_l, const uint8_t* mask_r, double* cov36,
                rsvio_motion_cov_info* info) {
    p.init_cov();
    const size_t n_l = (size_t)A.P.n[0], n_r = (size_t)A.P.n[1];
    if (mask_l && n_l) std::memcpy(p.hcmask.p, mask_l, n_l);
    if (mask_r && n_r) std::memcpy(p.hcmask.p + n_l, mask_r, n_r);
    if ((mask_l && n_l) || (mask_r && n_r))
        RSVIO_HIP(hipMemcpyAsync(p.cmask.p, p.hcmask.p, n_l + n_r, hipMemcpyHostToDevice, stream));
    A.mask[0] = mask_l ? p.cmask.p : nullptr;
    A.mask[1] = mask_r ? p.cmask.p + n_l : nullptr;
    A.out = p.hcov.p;
    hipLaunchKernelGGL(pnp_covariance_kernel, dim3(1), dim3(kPnpThreads), 0, stream, A);
    RSVIO_HIP(hipGetLastError());
    RSVIO_HIP(hipStreamSynchronize(stream));
    std::memcpy(cov36, p.hcov.p->cov, sizeof p.hcov.p->cov);
    *info = p.hcov.p->info;
    return RSVIO_OK;
}

// ---- batched motion tracking: one frame per handle, all in one launch chain ----

constexpr int kPnpBatchMax = 4096;       // handles per batch
constexpr int kPnpBatchSmallCap = 1024;  // the batched kernels' small LDS capacity (features)

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

struct PnpBatch {
    int device = 0, n = 0;
    std::vector<Pnp*> h;               // borrowed
    hipStream_t stream = nullptr;      // the batch's own
    hipEvent_t ev[2] = {nullptr, nullptr};
    // one image per call: the argument table, then every host frame's [ids_l | ids_r | uv_l | uv_r]
    // and (robust) the explicit samples, each at a 16-byte-aligned offset; one H2D copy moves it
    HostBuf<uint8_t> himg;
    DevBuf<uint8_t> dimg;
    std::vector<size_t> frame_off, samp_off;
    HostBuf<rsvio_motion_result> hres;             // the kernels' result table (plain)
    HostBuf<rsvio_robust_motion_result> hrobust;   // ... (robust)
    // the robust path's per-stream scratch (RobustBufs), allocated by the first robust run
    DevBuf<double> rdbl;
    DevBuf<int> rint;
    DevBuf<int> rcount;                // hyp_count: stream i at i * n_hyp
    DevBuf<uint8_t> rmask;             // mask: stream i at i * (the call's mask stride)
    HostBuf<int> hcount;
    HostBuf<uint8_t> hmask;
    HostBuf<CovOut> hcov;              // the covariance kernel's result table

    static constexpr size_t kDblPerStream = kRobustDbl, kIntPerStream = kRobustInt;

    void init(int dev, std::vector<Pnp*> handles) {
        device = dev;
        h = std::move(handles);
        n = (int)h.size();
        frame_off.resize(n);
        samp_off.resize(n);
        RSVIO_HIP(hipSetDevice(dev));
        RSVIO_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        RSVIO_HIP(hipEventCreate(&ev[0]));
        RSVIO_HIP(hipEventCreate(&ev[1]));
        hres.alloc(n);
    }
    void init_robust() {
        if (hrobust.p) return;
        rdbl.alloc(kDblPerStream * n);
        rint.alloc(kIntPerStream * n);
        rcount.alloc((size_t)kRansacMaxHyp * n);
        rmask.alloc((size_t)kPnpMaxFeatures * n);
        hrobust.alloc(n);
    }
    void reserve_image(size_t bytes) {  // (no copy is in flight: every run ends with a host wait)
        if (himg.n >= bytes) return;
        const size_t cap = bytes + bytes / 2;
        himg.alloc(cap);
        dimg.alloc(cap);
    }
    ~PnpBatch() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// The host-side checks of a batched call `who`: nothing is launched or written unless all pass.
// lm: a tracking call, whose slots need T_W_B_last_kf and a cfg (their own or the call's `cfg`);
// the covariance call reads neither
int batch_check(const PnpBatch& b, const rsvio_motion_frame* frames, const char* who, bool lm,
                const rsvio_lm_cfg* cfg = nullptr) {
    for (int i = 0; i < b.n; ++i) {
        const rsvio_motion_frame& f = frames[i];
        if ((lm && (!f.T_W_B_last_kf || (!f.cfg && !cfg))) || !f.T_C_B2 || (f.n_l && (!f.ids_l || !f.uv_l)) ||
            (f.n_r && (!f.ids_r || !f.uv_r)) || f.id_stride < 0 || (f.id_stride && f.id_stride < 8)) {
            char msg[96];
            std::snprintf(msg, sizeof msg, "%s: slot %d: a NULL argument%s or a bad id_stride", who, i,
                          lm ? ", no cfg" : "");
            set_last_error(msg);
            return RSVIO_ERR_INVALID_ARG;
        }
    }
    for (int i = 0; i < b.n; ++i)
        if (frames[i].n_l > (size_t)kPnpMaxFeatures || frames[i].n_r > (size_t)kPnpMaxFeatures ||
            frames[i].n_l + frames[i].n_r > (size_t)kPnpMaxFeatures) {
            char msg[96];
            std::snprintf(msg, sizeof msg, "%s: slot %d: more than 4096 features in one frame", who, i);
            set_last_error(msg);
            return RSVIO_ERR_CAPACITY;
        }
    return RSVIO_OK;
}

// The LDS capacity of this call's kernels: the small one when the batch's largest frame fits
// (several workgroups per CU), RSVIO_PNP_BATCH_CAP=4096 forcing the large one
int batch_cap(const PnpBatch& b, const rsvio_motion_frame* frames) {
    size_t most = 0;
    for (int i = 0; i < b.n; ++i) most = std::max(most, frames[i].n_l + frames[i].n_r);
    const char* e = std::getenv("RSVIO_PNP_BATCH_CAP");
    if (e && std::atoi(e) == kPnpMaxFeatures) return kPnpMaxFeatures;
    return most <= (size_t)kPnpBatchSmallCap ? kPnpBatchSmallCap : kPnpMaxFeatures;
}

// f(std::integral_constant<int, CAP>) for batch_cap's value: a kernel<CAP> has one launch site
template <class F>
void with_cap(int cap, F f) {
    if (cap == kPnpBatchSmallCap)
        f(std::integral_constant<int, kPnpBatchSmallCap>{});
    else
        f(std::integral_constant<int, kPnpMaxFeatures>{});
}

// A batched run's timed section on the batch's stream and events; the time also to *device_ms
template <class Launch, class Then = void (*)()>
float batch_timed(PnpBatch& b, double* device_ms, Launch launch, Then then = [] {}) {
    const float ms = timed_section(b.stream, b.ev, launch, then);
    if (device_ms) *device_ms = ms;
    return ms;
}

// Lay the call's image out (table of n entries of `entry` bytes, host frames, samples of
// `samp_bytes` each where given, then `extra` bytes the caller fills) and stage the host frames and
// samples; returns the size without the extra bytes, i.e. their offset
size_t batch_stage(PnpBatch& b, const rsvio_motion_frame* frames, size_t entry, size_t samp_bytes, size_t extra = 0) {
    size_t off = align16(entry * (size_t)b.n);
    for (int i = 0; i < b.n; ++i) {
        const rsvio_motion_frame& f = frames[i];
        b.frame_off[i] = off;
        if (!f.on_device) off += 16 * (f.n_l + f.n_r);
        b.samp_off[i] = off;
        if (samp_bytes && f.samples) off += align16(samp_bytes);
    }
    b.reserve_image(off + extra);
    for (int i = 0; i < b.n; ++i) {
        const rsvio_motion_frame& f = frames[i];
        if (!f.on_device) pack_frame(b.himg.p + b.frame_off[i], f.ids_l, f.uv_l, f.n_l, f.ids_r, f.uv_r, f.n_r);
        if (samp_bytes && f.samples) std::memcpy(b.himg.p + b.samp_off[i], f.samples, samp_bytes);
    }
    return off;
}

// Slot i's lists in A: device pointers read in place, or the frame staged in the call's image
void batch_lists(const PnpBatch& b, int i, const rsvio_motion_frame& f, PnpArgs& A) {
    packed_lists(b.dimg.p + b.frame_off[i], f.n_l, f.n_r, A);
    if (f.on_device) {  // device pointers, read in place
        A.ids[0] = reinterpret_cast<const uint8_t*>(f.ids_l);
        A.ids[1] = reinterpret_cast<const uint8_t*>(f.ids_r);
        A.id_stride = f.id_stride ? f.id_stride : 8;
        A.uv[0] = reinterpret_cast<const float2*>(f.uv_l);
        A.uv[1] = reinterpret_cast<const float2*>(f.uv_r);
    }
}

// Slot i's PnpArgs: handle i's current map, frame i's poses, cfg and lists
PnpArgs batch_args(PnpBatch& b, int i, const rsvio_motion_frame& f, const rsvio_lm_cfg* cfg,
                   const rsvio_keyframe_rule* rule) {
    PnpArgs A = make_args(*b.h[i], f.T_W_B_last_kf, f.T_C_B2, f.cfg ? f.cfg : cfg, rule);
    batch_lists(b, i, f, A);
    return A;
}

int run_pnp_batch(PnpBatch& b, const rsvio_motion_frame* frames, const rsvio_lm_cfg* cfg,
                  const rsvio_keyframe_rule* rule, rsvio_motion_result* results, double* device_ms) {
    RSVIO_HIP(hipSetDevice(b.device));
    const int cap = batch_cap(b, frames);
    const size_t bytes = batch_stage(b, frames, sizeof(PnpArgs), 0);
    PnpArgs* tab = reinterpret_cast<PnpArgs*>(b.himg.p);
    for (int i = 0; i < b.n; ++i) {
        tab[i] = batch_args(b, i, frames[i], cfg, rule);
        tab[i].out = b.hres.p + i;
    }
    RSVIO_HIP(hipMemcpyAsync(b.dimg.p, b.himg.p, bytes, hipMemcpyHostToDevice, b.stream));
    const PnpArgs* dtab = reinterpret_cast<const PnpArgs*>(b.dimg.p);
    batch_timed(
        b, device_ms,
        [&] {
            with_cap(cap, [&](auto c) {
                hipLaunchKernelGGL(pnp_track_motion_batch_kernel<decltype(c)::value>, dim3(b.n), dim3(kPnpThreads), 0,
                                   b.stream, dtab);
            });
        });
    for (int i = 0; i < b.n; ++i) {
        results[i] = b.hres.p[i];
        keyframe_rule(tab[i], &results[i]);
    }
    return RSVIO_OK;
}

int run_pnp_batch_robust(PnpBatch& b, const rsvio_motion_frame* frames, const rsvio_lm_cfg* cfg,
                         const rsvio_keyframe_rule* rule, const rsvio_ransac_cfg* rc,
                         rsvio_robust_motion_result* results, double* device_ms) {
    RSVIO_HIP(hipSetDevice(b.device));
    b.init_robust();
    const int cap = batch_cap(b, frames);
    const size_t n_hyp = (size_t)rc->n_hyp;
    const size_t bytes = batch_stage(b, frames, sizeof(RobustArgs), sizeof(int32_t) * 3 * n_hyp);
    size_t most = 0;
    bool want_mask = false, want_count = false;
    for (int i = 0; i < b.n; ++i) {
        most = std::max(most, frames[i].n_l + frames[i].n_r);
        want_mask |= frames[i].mask_l || frames[i].mask_r;
        want_count |= frames[i].hyp_count != nullptr;
    }
    const size_t mstride = align16(most);
    RobustArgs* tab = reinterpret_cast<RobustArgs*>(b.himg.p);
    for (int i = 0; i < b.n; ++i) {
        RobustArgs RA{};
        RA.P = batch_args(b, i, frames[i], cfg, rule);
        RA.P.out = &b.hrobust.p[i].motion;
        RA.B = robust_carve(b.rdbl.p + PnpBatch::kDblPerStream * i, b.rint.p + PnpBatch::kIntPerStream * i);
        RA.B.hyp_count = b.rcount.p + n_hyp * i;
        RA.B.samples = frames[i].samples ? reinterpret_cast<const int*>(b.dimg.p + b.samp_off[i]) : nullptr;
        RA.B.mask = b.rmask.p + mstride * i;
        set_ransac(RA, rc);
        RA.out = b.hrobust.p + i;
        tab[i] = RA;
    }
    if (want_mask && b.hmask.n < mstride * b.n) b.hmask.alloc(mstride * b.n);
    if (want_count && b.hcount.n < n_hyp * b.n) b.hcount.alloc(n_hyp * b.n);
    RSVIO_HIP(hipMemcpyAsync(b.dimg.p, b.himg.p, bytes, hipMemcpyHostToDevice, b.stream));
    const RobustArgs* dtab = reinterpret_cast<const RobustArgs*>(b.dimg.p);
    const float ms = batch_timed(
        b, device_ms,
        [&] {
            with_cap(cap, [&](auto c) {
                constexpr int CAP = decltype(c)::value;
                hipLaunchKernelGGL(pnp_robust_join_batch_kernel<CAP>, dim3(b.n), dim3(kPnpThreads), 0, b.stream, dtab);
                hipLaunchKernelGGL(pnp_robust_score_batch_kernel, dim3(rc->n_hyp, b.n), dim3(64), 0, b.stream, dtab);
                hipLaunchKernelGGL(pnp_robust_refit_batch_kernel<CAP>, dim3(b.n), dim3(kPnpThreads), 0, b.stream, dtab);
            });
        },
        [&] {
            if (want_mask && mstride)
                RSVIO_HIP(hipMemcpyAsync(b.hmask.p, b.rmask.p, mstride * b.n, hipMemcpyDeviceToHost, b.stream));
            if (want_count)
                RSVIO_HIP(hipMemcpyAsync(b.hcount.p, b.rcount.p, sizeof(int32_t) * n_hyp * b.n, hipMemcpyDeviceToHost,
                                         b.stream));
        });
    for (int i = 0; i < b.n; ++i) {
        const rsvio_motion_frame& f = frames[i];
        results[i] = b.hrobust.p[i];
        keyframe_rule(tab[i].P, &results[i].motion);
        results[i].device_ms = ms;
        const uint8_t* m = b.hmask.p + mstride * i;
        if (f.mask_l && f.n_l) std::memcpy(f.mask_l, m, f.n_l);
        if (f.mask_r && f.n_r) std::memcpy(f.mask_r, m + f.n_l, f.n_r);
        if (f.hyp_count) std::memcpy(f.hyp_count, b.hcount.p + n_hyp * i, sizeof(int32_t) * n_hyp);
    }
    return RSVIO_OK;
}

// One upload (the argument table, the host frames, the masks), one launch on a grid of n, one wait
int run_pnp_batch_cov(PnpBatch& b, const rsvio_motion_frame* frames, const double* T_W_B, double huber_delta,
                      double* cov, rsvio_motion_cov_info* info, double* device_ms) {
    RSVIO_HIP(hipSetDevice(b.device));
    if (!b.hcov.p) b.hcov.alloc(b.n);
    size_t mbytes = 0;  // a slot's masks as [mask_l | mask_r], each slot at a 16-byte-aligned offset
    for (int i = 0; i < b.n; ++i)
        if (frames[i].mask_l || frames[i].mask_r) mbytes += align16(frames[i].n_l + frames[i].n_r);
    const size_t moff = batch_stage(b, frames, sizeof(CovArgs), 0, mbytes);
    CovArgs* tab = reinterpret_cast<CovArgs*>(b.himg.p);
    size_t off = moff;
    for (int i = 0; i < b.n; ++i) {
        const rsvio_motion_frame& f = frames[i];
        CovArgs A = cov_args(*b.h[i], T_W_B + 16 * i, f.T_C_B2, huber_delta);
        batch_lists(b, i, f, A.P);
        if (f.mask_l || f.mask_r) {
            if (f.mask_l && f.n_l) std::memcpy(b.himg.p + off, f.mask_l, f.n_l);
            if (f.mask_r && f.n_r) std::memcpy(b.himg.p + off + f.n_l, f.mask_r, f.n_r);
            A.mask[0] = f.mask_l ? b.dimg.p + off : nullptr;
            A.mask[1] = f.mask_r ? b.dimg.p + off + f.n_l : nullptr;
            off += align16(f.n_l + f.n_r);
        }
        A.out = b.hcov.p + i;
        tab[i] = A;
    }
    RSVIO_HIP(hipMemcpyAsync(b.dimg.p, b.himg.p, moff + mbytes, hipMemcpyHostToDevice, b.stream));
    batch_timed(
        b, device_ms,
        [&] {
            hipLaunchKernelGGL(pnp_covariance_batch_kernel, dim3(b.n), dim3(kPnpThreads), 0, b.stream,
                               reinterpret_cast<const CovArgs*>(b.dimg.p));
        });
    for (int i = 0; i < b.n; ++i) {
        std::memcpy(cov + 36 * (size_t)i, b.hcov.p[i].cov, sizeof b.hcov.p[i].cov);
        info[i] = b.hcov.p[i].info;
    }
    return RSVIO_OK;
}

}  // namespace rsvio

struct rsvio_pnp {
    rsvio::Pnp p;
};

struct rsvio_pnp_batch {
    rsvio::PnpBatch b;
};

using rsvio::guarded;

extern "C" {

int rsvio_quat_from_matrix(const double* R, size_t n, double* q) {
    if (n && (!R || !q)) return RSVIO_ERR_INVALID_ARG;
    for (size_t i = 0; i < n; ++i) rsvio::rot::quat_from_matrix(R + 9 * i, q + 4 * i);
    return RSVIO_OK;
}

int rsvio_pnp_create(int32_t device, rsvio_pnp** out) {
    if (!out) return RSVIO_ERR_INVALID_ARG;
    return guarded([&] {
        auto* h = new rsvio_pnp();
        try {
            h->p.init(device);
        } catch (...) {
            delete h;
            throw;
        }
        *out = h;
        return (int)RSVIO_OK;
    });
}

void rsvio_pnp_destroy(rsvio_pnp* p) { delete p; }

int rsvio_pnp_set_stream(rsvio_pnp* h, void* stream) {
    if (!h) return RSVIO_ERR_INVALID_ARG;
    return guarded([&] {
        RSVIO_HIP(hipStreamSynchronize(h->p.active()));
        h->p.user = static_cast<hipStream_t>(stream);
        return (int)RSVIO_OK;
    });
}

int rsvio_pnp_set_map(rsvio_pnp* h, const uint64_t* ids, const float* p_W, int32_t n) {
    if (!h || n < 0 || (n && (!ids || !p_W))) return RSVIO_ERR_INVALID_ARG;
    for (int32_t i = 1; i < n; ++i)
        if (!(ids[i - 1] < ids[i])) {
            rsvio::set_last_error("rsvio_pnp_set_map: ids must be strictly ascending");
            return RSVIO_ERR_INVALID_ARG;
        }
    return guarded([&] {
        auto& P = h->p;
        RSVIO_HIP(hipSetDevice(P.device));
        // the hash table: >= 4 n entries (load <= 1/4: a bucket overflows into the next one for
        // well under 1 % of the ids), linear probing over buckets
        int nb = 16;
        while ((size_t)nb * rsvio::kBucket < (size_t)4 * n) nb *= 2;
        P.htable.assign((size_t)nb * rsvio::kBucket, rsvio::PnpEntry{rsvio::kEmptyId, {0.f, 0.f, 0.f}, 0u});
        P.bucket_mask = nb - 1;
        P.max_probe = 0;
        P.has_top = 0;
        for (int32_t i = 0; i < n; ++i) {
            if (ids[i] == rsvio::kEmptyId) {  // the one id the table cannot hold (the largest: last)
                P.has_top = 1;
                for (int k = 0; k < 3; ++k) P.top_pw[k] = p_W[3 * i + k];
                continue;
            }
            uint32_t b = rsvio::map_bucket(ids[i], P.bucket_mask);
            for (int probe = 0;; ++probe) {
                rsvio::PnpEntry* e = &P.htable[(size_t)b * rsvio::kBucket];
                int k = 0;
                while (k < rsvio::kBucket && e[k].id != rsvio::kEmptyId) ++k;
                if (k < rsvio::kBucket) {
                    e[k].id = ids[i];
                    for (int c = 0; c < 3; ++c) e[k].pw[c] = p_W[3 * i + c];
                    P.max_probe = std::max(P.max_probe, probe);
                    break;
                }
                b = (b + 1) & (uint32_t)P.bucket_mask;
            }
        }
        if (P.table.n < P.htable.size()) P.table.alloc(P.htable.size());
        RSVIO_HIP(hipMemcpyAsync(P.table.p, P.htable.data(), sizeof(rsvio::PnpEntry) * P.htable.size(),
                                 hipMemcpyHostToDevice, P.active()));
        RSVIO_HIP(hipStreamSynchronize(P.active()));
        P.n_map = n;
        return (int)RSVIO_OK;
    });
}

// Diagnostic (host only, not part of the ABI header): the shape of the table the last set_map
// built -> {buckets, max_probe, has_top, n_map}
int rsvio_dbg_pnp_map_stats(rsvio_pnp* h, int32_t out[4]) {
    if (!h || !out) return RSVIO_ERR_INVALID_ARG;
    const auto& P = h->p;
    out[0] = (int32_t)(P.htable.size() / rsvio::kBucket);
    out[1] = P.max_probe;
    out[2] = P.has_top;
    out[3] = P.n_map;
    return RSVIO_OK;
}

int rsvio_track_motion(rsvio_pnp* h, const uint64_t* ids_l, const float* uv_l, size_t n_l, const uint64_t* ids_r,
                       const float* uv_r, size_t n_r, const double* T_W_B_last_kf, const double* T_C_B2,
                       const rsvio_lm_cfg* cfg, const rsvio_keyframe_rule* rule, rsvio_motion_result* res) {
    if (!h || !T_W_B_last_kf || !T_C_B2 || !cfg || !rule || !res || (n_l && (!ids_l || !uv_l)) ||
        (n_r && (!ids_r || !uv_r)))
        return RSVIO_ERR_INVALID_ARG;
    if (n_l + n_r > (size_t)rsvio::kPnpMaxFeatures) {
        rsvio::set_last_error("track_motion: more than 4096 features in one frame");
        return RSVIO_ERR_CAPACITY;
    }
    return guarded([&] {
        auto& P = h->p;
        RSVIO_HIP(hipSetDevice(P.device));
        rsvio::PnpArgs A = rsvio::make_args(P, T_W_B_last_kf, T_C_B2, cfg, rule);
        rsvio::host_frame(P, ids_l, uv_l, n_l, ids_r, uv_r, n_r, A);
        return rsvio::run_pnp(P, A, P.active(), res);
    });
}

int rsvio_track_motion_tracker(rsvio_pnp* h, rsvio_tracker* t, const double* T_W_B_last_kf, const double* T_C_B2,
                               const rsvio_lm_cfg* cfg, const rsvio_keyframe_rule* rule, rsvio_motion_result* res) {
    if (!h || !t || !T_W_B_last_kf || !T_C_B2 || !cfg || !rule || !res) return RSVIO_ERR_INVALID_ARG;
    return guarded([&] {
        auto& P = h->p;
        rsvio::PnpArgs A = rsvio::make_args(P, T_W_B_last_kf, T_C_B2, cfg, rule);
        const int rc = rsvio::tracker_frame(P, t, A);
        if (rc != RSVIO_OK) return rc;
        return rsvio::run_pnp(P, A, P.active(), res);
    });
}

int rsvio_track_motion_robust(rsvio_pnp* h, const uint64_t* ids_l, const float* uv_l, size_t n_l, const uint64_t* ids_r,
                              const float* uv_r, size_t n_r, const double* T_W_B_last_kf, const double* T_C_B2,
                              const rsvio_lm_cfg* cfg, const rsvio_keyframe_rule* rule, const rsvio_ransac_cfg* ransac,
                              const int32_t* samples, uint8_t* mask_l, uint8_t* mask_r, int32_t* hyp_count,
                              rsvio_robust_motion_result* res) {
    if (!h || !T_W_B_last_kf || !T_C_B2 || !cfg || !rule || !res || (n_l && (!ids_l || !uv_l)) ||
        (n_r && (!ids_r || !uv_r)) || !rsvio::ransac_cfg_ok(ransac))
        return RSVIO_ERR_INVALID_ARG;
    if (n_l + n_r > (size_t)rsvio::kPnpMaxFeatures) {
        rsvio::set_last_error("track_motion: more than 4096 features in one frame");
        return RSVIO_ERR_CAPACITY;
    }
    return guarded([&] {
        auto& P = h->p;
        RSVIO_HIP(hipSetDevice(P.device));
        rsvio::PnpArgs A = rsvio::make_args(P, T_W_B_last_kf, T_C_B2, cfg, rule);
        rsvio::host_frame(P, ids_l, uv_l, n_l, ids_r, uv_r, n_r, A);
        return rsvio::run_pnp_robust(P, A, P.active(), ransac, samples, mask_l, mask_r, hyp_count, res);
    });
}

int rsvio_track_motion_robust_tracker(rsvio_pnp* h, rsvio_tracker* t, const double* T_W_B_last_kf,
                                      const double* T_C_B2, const rsvio_lm_cfg* cfg, const rsvio_keyframe_rule* rule,
                                      const rsvio_ransac_cfg* ransac, const int32_t* samples, uint8_t* mask_l,
                                      uint8_t* mask_r, int32_t* hyp_count, rsvio_robust_motion_result* res) {
    if (!h || !t || !T_W_B_last_kf || !T_C_B2 || !cfg || !rule || !res || !rsvio::ransac_cfg_ok(ransac))
        return RSVIO_ERR_INVALID_ARG;
    return guarded([&] {
        auto& P = h->p;
        rsvio::PnpArgs A = rsvio::make_args(P, T_W_B_last_kf, T_C_B2, cfg, rule);
        const int rc = rsvio::tracker_frame(P, t, A);
        if (rc != RSVIO_OK) return rc;
        return rsvio::run_pnp_robust(P, A, P.active(), ransac, samples, mask_l, mask_r, hyp_count, res);
    });
}

int rsvio_pnp_batch_create(rsvio_pnp* const* handles, int32_t n, rsvio_pnp_batch** out) {
    if (!handles || !out || n < 1 || n > rsvio::kPnpBatchMax) return RSVIO_ERR_INVALID_ARG;
    std::vector<rsvio::Pnp*> h((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        if (!handles[i]) return RSVIO_ERR_INVALID_ARG;
        h[i] = &handles[i]->p;
        if (h[i]->device != h[0]->device) {
            rsvio::set_last_error("rsvio_pnp_batch_create: the handles are on different devices");
            return RSVIO_ERR_INVALID_ARG;
        }
    }
    return guarded([&] {
        auto* b = new rsvio_pnp_batch();
        try {
            b->b.init(h[0]->device, std::move(h));
        } catch (...) {
            delete b;
            throw;
        }
        *out = b;
        return (int)RSVIO_OK;
    });
}

void rsvio_pnp_batch_destroy(rsvio_pnp_batch* b) { delete b; }

int rsvio_pnp_batch_track_motion(rsvio_pnp_batch* b, const rsvio_motion_frame* frames, const rsvio_lm_cfg* cfg,
                                 const rsvio_keyframe_rule* rule, rsvio_motion_result* results, double* device_ms) {
    if (!b || !frames || !rule || !results) return RSVIO_ERR_INVALID_ARG;
    const int rc = rsvio::batch_check(b->b, frames, "rsvio_pnp_batch_track_motion", true, cfg);
    if (rc != RSVIO_OK) return rc;
    return guarded([&] { return rsvio::run_pnp_batch(b->b, frames, cfg, rule, results, device_ms); });
}

int rsvio_pnp_batch_track_motion_robust(rsvio_pnp_batch* b, const rsvio_motion_frame* frames, const rsvio_lm_cfg* cfg,
                                        const rsvio_keyframe_rule* rule, const rsvio_ransac_cfg* ransac,
                                        rsvio_robust_motion_result* results, double* device_ms) {
    if (!b || !frames || !rule || !results || !rsvio::ransac_cfg_ok(ransac)) return RSVIO_ERR_INVALID_ARG;
    const int rc = rsvio::batch_check(b->b, frames, "rsvio_pnp_batch_track_motion_robust", true, cfg);
    if (rc != RSVIO_OK) return rc;
    return guarded(
        [&] { return rsvio::run_pnp_batch_robust(b->b, frames, cfg, rule, ransac, results, device_ms); });
}

int rsvio_motion_covariance(rsvio_pnp* h, const uint64_t* ids_l, const float* uv_l, size_t n_l, const uint64_t* ids_r,
                            const float* uv_r, size_t n_r, const uint8_t* mask_l, const uint8_t* mask_r,
                            const double* T_W_B, const double* T_C_B2, double huber_delta, double* cov36,
                            rsvio_motion_cov_info* info) {
    if (!h || !T_W_B || !T_C_B2 || !cov36 || !info || (n_l && (!ids_l || !uv_l)) || (n_r && (!ids_r || !uv_r)) ||
        !(huber_delta > 0.0))  // (NaN fails >)
        return RSVIO_ERR_INVALID_ARG;
    if (n_l > (size_t)rsvio::kPnpMaxFeatures || n_r > (size_t)rsvio::kPnpMaxFeatures ||
        n_l + n_r > (size_t)rsvio::kPnpMaxFeatures) {
        rsvio::set_last_error("motion_covariance: more than 4096 features in one frame");
        return RSVIO_ERR_CAPACITY;
    }
    return guarded([&] {
        auto& P = h->p;
        RSVIO_HIP(hipSetDevice(P.device));
        rsvio::CovArgs A = rsvio::cov_args(P, T_W_B, T_C_B2, huber_delta);
        rsvio::host_frame(P, ids_l, uv_l, n_l, ids_r, uv_r, n_r, A.P);
        return rsvio::run_pnp_cov(P, A, P.active(), mask_l, mask_r, cov36, info);
    });
}

int rsvio_motion_covariance_tracker(rsvio_pnp* h, rsvio_tracker* t, const uint8_t* mask_l, const uint8_t* mask_r,
                                    const double* T_W_B, const double* T_C_B2, double huber_delta, double* cov36,
                                    rsvio_motion_cov_info* info) {
    if (!h || !t || !T_W_B || !T_C_B2 || !cov36 || !info || !(huber_delta > 0.0)) return RSVIO_ERR_INVALID_ARG;
    return guarded([&] {
        auto& P = h->p;
        rsvio::CovArgs A = rsvio::cov_args(P, T_W_B, T_C_B2, huber_delta);
        const int rc = rsvio::tracker_frame(P, t, A.P);
        if (rc != RSVIO_OK) return rc;
        return rsvio::run_pnp_cov(P, A, P.active(), mask_l, mask_r, cov36, info);
    });
}

int rsvio_pnp_batch_covariance(rsvio_pnp_batch* b, const rsvio_motion_frame* frames, const double* T_W_B,
                               double huber_delta, double* cov, rsvio_motion_cov_info* info, double* device_ms) {
    if (!b || !frames || !T_W_B || !cov || !info || !(huber_delta > 0.0)) return RSVIO_ERR_INVALID_ARG;
    const int rc = rsvio::batch_check(b->b, frames, "rsvio_pnp_batch_covariance", false);
    if (rc != RSVIO_OK) return rc;
    return guarded([&] { return rsvio::run_pnp_batch_cov(b->b, frames, T_W_B, huber_delta, cov, info, device_ms); });
}

}  // extern "C"
