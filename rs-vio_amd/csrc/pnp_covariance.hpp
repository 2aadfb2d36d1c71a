// pnp_covariance.hpp -- the 6x6 covariance of a tracked frame's pose (rsvio_motion_covariance*,
// rsvio_pnp_batch_covariance).  Included by pnp.hip inside its file-local namespace, after
// pnp_robust.hpp: it reuses that file's PnpArgs (the lists and the map table), map_lookup,
// pnp_linearize_cw, pnp_huber and wave_reduce_scatter32, and leaves every other kernel as it is.
//
// Definition (include/rsvio_gpu.h): at x = T_B_W = inverse(T_W_B) of the pose the caller passes,
//   H = sum over the factors of w J^T J,  Sigma = H^-1,
// J the PnP factor's 2x6 [dt | dw] (pnp_linearize_cw), w the Huber IRLS weight at huber_delta, no
// damping, in the tangent of the LM's (+) (se3_plus_r: T_B_W <- T_B_W Exp([dt; dw])).  A feature of
// the left list, then of the right list, is a factor iff its id has a map point (map_lookup) and
// its mask byte is 1 (or that list has no mask).
//
// One launch, one workgroup of kPnpThreads per frame, one pass: no LM loop, so nothing is staged
// in LDS.  Lane t takes the features t, t + 512, ... of the left list, then of the right list,
// and keeps H's upper 21 entries, the cost and the two counts in registers; the waves reduce by
// the DPP reduce-scatter, then in wave order through LDS; wave 0 factorises H = L D L^T and solves
// the six unit right-hand sides with IEEE divisions (one factorisation per call: accuracy before
// the reciprocal trick of the LM's serial chain).  Every sum has a fixed order, so two calls give
// the same bits and a batch slot gives the single call's.
#pragma once

constexpr int kCovRed = 22;  // H upper (21), cost

struct CovOut {  // pinned host memory, one per frame
    double cov[36];
    rsvio_motion_cov_info info;
};

struct CovArgs {
    PnpArgs P;               // the lists, the map table and wclk_khz (nothing else is read)
    const uint8_t* mask[2];  // device: one byte per feature of that list (1: use), or null: every one
    double TCW[2][12];       // T_C_W = T_C_B T_B_W per camera (R row-major, then t), host f64
    double huber_delta;
    CovOut* out;
};

// H^-1 by LDL^T (H's upper triangle packed as utri6) with IEEE divisions, every index a
// compile-time constant (registers).  false: pivot `*bad` is not positive and finite -- the rule
// of ldl6 and of the BA covariance; S then holds nothing.  S is written to (r, c) and (c, r) from
// one value: symmetric bit for bit.
__device__ __forceinline__ bool cov_invert6(const double (&Hp)[21], double (&S)[36], double* min_pivot) {
    double L[6][6], U[6][6], d[6];
    bool ok = true;
    double pmin = 0.0, bad = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double p = Hp[utri6(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) p -= L[j][k] * U[j][k];
        const bool good = (p > 0.0) && isfinite(p);
        if (ok && !good) bad = p;               // the first pivot that failed
        pmin = (j == 0 || p < pmin) ? p : pmin;
        ok &= good;
        d[j] = p;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double u = Hp[utri6(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) u -= L[i][k] * U[j][k];
            U[i][j] = u;
            L[i][j] = u / p;
        }
    }
    *min_pivot = ok ? pmin : bad;
    if (!ok) return false;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        // L z = e_c (z_i = 0 for i < c), y = z / d, L^T x = y
        double z[6], x[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double s = (i == c) ? 1.0 : 0.0;
#pragma unroll
            for (int k = c; k < i; ++k) s -= L[i][k] * z[k];
            z[i] = s;
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {
            double s = (i >= c) ? z[i] / d[i] : 0.0;
#pragma unroll
            for (int k = i + 1; k < 6; ++k) s -= L[k][i] * x[k];
            x[i] = s;
        }
#pragma unroll
        for (int r = 0; r <= c; ++r) {
            S[6 * r + c] = x[r];
            S[6 * c + r] = x[r];
        }
    }
    return true;
}

__device__ __forceinline__ void pnp_covariance_body(const CovArgs& A) {
    __shared__ double s_tcw[2][12];
    __shared__ double s_red[kPnpWaves][kCovRed];
    __shared__ int s_cnt[kPnpWaves][2];
    __shared__ double s_sum[kCovRed];
    __shared__ double s_cov[36];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned long long t_entry = wall_clock64();
    if (tid < 24) s_tcw[tid / 12][tid % 12] = A.TCW[tid / 12][tid % 12];
    __syncthreads();  // T_C_W
    double acc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.0;
    int n_obs = 0, n_down = 0;
    const bool have_map = A.P.n_map > 0;
#pragma unroll 1
    for (int cam = 0; cam < 2; ++cam) {
        const uint8_t* ids = A.P.ids[cam];
        const float2* uvs = A.P.uv[cam];
        const uint8_t* mask = A.mask[cam];
        const int n = have_map ? A.P.n[cam] : 0;
#pragma unroll 1
        for (int i = tid; i < n; i += kPnpThreads) {
            if (mask && mask[i] != 1) continue;
            const uint64_t id = *reinterpret_cast<const uint64_t*>(ids + (size_t)i * A.P.id_stride);
            const float2 q = uvs[i];
            float pw[3];
            if (!map_lookup(A.P, id, pw)) continue;
            const double pW[3] = {(double)pw[0], (double)pw[1], (double)pw[2]};
            const double uv[2] = {(double)q.x, (double)q.y};
            double r[2], J[2][6];
            pnp_linearize_cw(pW, uv, s_tcw[cam], r, J);
            const double s2 = r[0] * r[0] + r[1] * r[1];
            double rho, w;
            pnp_huber(s2, A.huber_delta, &rho, &w);
            acc[21] += 0.5 * rho;
            ++n_obs;
            n_down += (w < 1.0) ? 1 : 0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double w0 = w * J[0][a], w1 = w * J[1][a];
#pragma unroll
                for (int c = a; c < 6; ++c) acc[utri6(a, c)] += w0 * J[0][c] + w1 * J[1][c];
            }
        }
    }
    {
        const double v = wave_reduce_scatter32(acc, lane);
        if ((lane & 1) == 0 && (lane >> 1) < kCovRed) s_red[wv][lane >> 1] = v;
    }
    for (int off = 32; off > 0; off >>= 1) {  // (integers: any order)
        n_obs += __shfl_xor(n_obs, off);
        n_down += __shfl_xor(n_down, off);
    }
    if (lane == 0) {
        s_cnt[wv][0] = n_obs;
        s_cnt[wv][1] = n_down;
    }
    __syncthreads();  // every wave's partials
    if (wv != 0) return;
    if (lane < kCovRed) {  // the waves in order (lane k sums value k)
        double v = s_red[0][lane];
#pragma unroll
        for (int w = 1; w < kPnpWaves; ++w) v += s_red[w][lane];
        s_sum[lane] = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // every lane of wave 0 the same values from here on
    int nobs = 0, ndown = 0;
#pragma unroll
    for (int w = 0; w < kPnpWaves; ++w) {
        nobs += s_cnt[w][0];
        ndown += s_cnt[w][1];
    }
    double H[21], S[36], min_pivot = 0.0;
#pragma unroll
    for (int k = 0; k < 21; ++k) H[k] = s_sum[k];
    int status = RSVIO_MCOV_OK;
    if (nobs < 3) {
        status = RSVIO_MCOV_TOO_FEW;
    } else if (!cov_invert6(H, S, &min_pivot)) {
        status = RSVIO_MCOV_SINGULAR;
    }
    if (lane == 0) {
        const double nan = __longlong_as_double(0x7FF8000000000000ll);
#pragma unroll
        for (int k = 0; k < 36; ++k) s_cov[k] = status == RSVIO_MCOV_OK ? S[k] : nan;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < 36) A.out->cov[lane] = s_cov[lane];
    if (lane == 0) {
        rsvio_motion_cov_info r;
        r.status = status;
        r.n_observations = nobs;
        r.n_downweighted = ndown;
        r.reserved = 0;
        r.cost = s_sum[21];
        r.min_pivot = min_pivot;
        r.kernel_ms = (double)(wall_clock64() - t_entry) / A.P.wclk_khz;
        A.out->info = r;
    }
}

__global__ __launch_bounds__(kPnpThreads) void pnp_covariance_kernel(CovArgs A) { pnp_covariance_body(A); }

// Batched: workgroup blockIdx.x is slot i, its arguments entry i of a table in device memory (as
// pnp_track_motion_batch_kernel).  No workgroup reads what another writes.
__global__ __launch_bounds__(kPnpThreads) void pnp_covariance_batch_kernel(const CovArgs* __restrict__ table) {
    pnp_covariance_body(table[blockIdx.x]);
}
