// ba_covariance.hpp -- pose and landmark covariance from the reduced camera system
// (rsvio_ba_covariance).  Included by ba.hip inside its file-local namespace: it uses that file's
// Geometry / Prob / Work types, the slot records, K4c and the camera solve's factorisations.
//
// x is the state rsvio_ba_get_state would return.  H = sum_obs w J^T J is the Gauss-Newton
// Hessian of the BA cost at x with no damping (lambda = 0): J the 2x9 [dp_W | dt | dw] of
// factors.rs:350-447 (zero on its cheirality branch), w the Huber IRLS weight, the pose columns
// the free keyframes' in ascending order in the tangent of se3_plus ([dt; dw] of T_B_W).
//   pose covariance      Sigma_cc    = S^-1,  S = U - W V^-1 W^T            (n = 6 n_free <= 120)
//   landmark covariance  Sigma_pp(l) = V_l^-1 + sum_{a,b} Y_a^T Sigma_cc[a,b] Y_b,  Y_k = W_k V_l^-1
// over the landmark's slots in free keyframes.  Units: normalised-image-coordinate^2 per unit
// measurement variance.
//
// Launch chain (one stream, no host wait in between):
//   ba_linearize            the existing K4 on a by-value Work whose "initial state" is x and whose
//                           state buffers, LM state and stamp are the call's own scratch: x is
//                           linearised into raw buffer 0, the reset K4 folds in lands in scratch
//   ba_schur_chunks         the existing K4c on an LM state of its own {lambda 0, nothing pending}:
//                           no decision is taken, the handle's LM states are not touched
//   ba_camera_covariance    one workgroup: the partial systems summed and scattered into LDS as K5
//                           does, the solver's own LDL^T (8-column panels up to 10 free keyframes,
//                           6x6 block pivots past that), then Sigma = L^-T D^-1 L^-1
//   ba_landmark_covariance  K6's decomposition: one wave per landmark group, lane = slot
//
// The inverse: wave w takes the 16-column blocks J = w, w + nw, ... of Sigma.  Its block column
// X = Sigma E_J lives in registers as 16x16 tiles in the matrix core's accumulator layout, which
// is also the layout of the B operand of v_mfma_f64_16x16x4f64 (register m of a tile = the k-chunk
// m), so a finished tile feeds the next update without a shuffle:
//   forward   Y_i = L_ii^-1 (E_i - sum_{J<=k<i} L_ik Y_k)      i = J .. NT-1
//   scale     Y  <- D^-1 Y
//   backward  X_i = L_ii^-T (Y_i - sum_{k>i} L_ki^T X_k)       i = NT-1 .. J
// The off-diagonal tile products run on the matrix cores (L read from LDS as the A operand); the
// unit-triangular 16x16 diagonal solves run on the VALU, a row at a time by cross-lane reads.
// Only the tiles on and below the diagonal are formed (the lower triangle), each value is stored
// to (r, c) and (c, r): Sigma_cc is symmetric bit for bit.  No second dense matrix: the factor
// stays in LDS where the solver left it, the block column is 4 registers per tile.
// Every sum has a fixed order: two calls give the same bits.
#pragma once

// cst[0]: the camera factor (1 inverted, -1 a pivot was not positive and finite), cst[1]: the
// landmarks with observations whose V is singular at lambda = 0
struct CovOut {
    double* cc;    // n x n row-major
    double* lm;    // n_lm x 9
    unsigned char* flags;  // n_lm
    double* cost;  // 1
    int* cst;
};

// K5's combine at lambda = 0: the kGrp partial systems summed in slot order, scattered into the
// dense LDS matrix by the window's map (the b row goes along, g_c is dropped)
template <int T>
__device__ __forceinline__ void cov_combine(const Geometry& G, const Prob& Pr, const Work& Wk, double* M) {
    const int ne = G.n_pb * 36 + 6 * G.n_free;
    const size_t L = sys_len(G);
    for (int e = threadIdx.x; e < ne; e += T) {
        const int d = Pr.dmap[e];
        double a = Wk.cpart[e];
#pragma unroll
        for (int x = 1; x < kGrp; ++x) a += Wk.cpart[(size_t)x * L + e];
        if (d >= 0) M[d & (kMfMapLambda - 1)] = a;
    }
}

// Sigma = L^-T D^-1 L^-1 from the factor in LDS: Lm column-major with leading dimension LD, unit
// lower, valid strictly below the diagonal for rows and columns < NP; dinv = 1 / D (zero past
// NP); n <= NP real rows (the rest is identity padding).
// Block column J by one wave (J a template parameter: every tile index is a compile-time
// constant, so the block column stays in registers).
template <int NP, int LD, int J>
__device__ __forceinline__ void cov_inverse_column(const double* Lm, const double* dinv, int n, double* cc, int lane) {
    constexpr int NT = (NP + 15) / 16;
    const int i16 = lane & 15, k4 = lane >> 4;
    {
        mf_dbl4 y[NT];
#pragma unroll
        for (int i = J; i < NT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) y[i][r] = (i == J && k4 + 4 * r == i16) ? 1.0 : 0.0;
        // forward: L Y = E_J
#pragma unroll
        for (int i = J; i < NT; ++i) {
#pragma unroll
            for (int k = J; k < i; ++k) {
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int r = 16 * i + i16, c = 16 * k + 4 * m + k4;  // c < r
                    const double a = r < NP ? -Lm[c * LD + r] : 0.0;
                    y[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, y[k][m], y[i], 0, 0, 0);
                }
            }
#pragma unroll
            for (int p = 0; p < 16; ++p) {  // the diagonal tile: row p is final, the rows below take it
                const double yp = __shfl(y[i][p >> 2], i16 + 16 * (p & 3));
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = k4 + 4 * r;
                    const double l = (q > p && 16 * i + q < NP) ? Lm[(16 * i + p) * LD + 16 * i + q] : 0.0;
                    y[i][r] = fma(-l, yp, y[i][r]);
                }
            }
        }
#pragma unroll
        for (int i = J; i < NT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) y[i][r] *= dinv[16 * i + k4 + 4 * r];
        // backward: L^T X = Y, the tile rows from the last up to the diagonal's
#pragma unroll
        for (int i = NT - 1; i >= J; --i) {
#pragma unroll
            for (int k = i + 1; k < NT; ++k) {
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int r = 16 * k + 4 * m + k4, c = 16 * i + i16;  // L[r][c], c < r
                    const double a = r < NP ? -Lm[c * LD + r] : 0.0;
                    y[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, y[k][m], y[i], 0, 0, 0);
                }
            }
#pragma unroll
            for (int p = 15; p >= 0; --p) {  // row p is final, the rows above take it
                const double xp = __shfl(y[i][p >> 2], i16 + 16 * (p & 3));
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = k4 + 4 * r;
                    const double l = (q < p && 16 * i + p < NP) ? Lm[(16 * i + q) * LD + 16 * i + p] : 0.0;
                    y[i][r] = fma(-l, xp, y[i][r]);
                }
            }
        }
        // the lower triangle and its mirror
#pragma unroll
        for (int i = J; i < NT; ++i) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * i + k4 + 4 * r, col = 16 * J + i16;
                if (row < n && col <= row) {
                    cc[(size_t)row * n + col] = y[i][r];
                    cc[(size_t)col * n + row] = y[i][r];
                }
            }
        }
    }
}

// every lane of every wave: wave w takes the block columns J = w, w + NW, ...
template <int NP, int LD, int NW, int J = 0>
__device__ __forceinline__ void cov_inverse_columns(const double* Lm, const double* dinv, int n, double* cc, int lane,
                                                    int wave) {
    if constexpr (J < (NP + 15) / 16) {
        if (wave == J % NW && 16 * J < n) cov_inverse_column<NP, LD, J>(Lm, dinv, n, cc, lane);
        cov_inverse_columns<NP, LD, NW, J + 1>(Lm, dinv, n, cc, lane, wave);
    }
}

// The two bodies are force-inlined into their kernels, as camera_solve_blk_body is: out of line
// the 16- and 20-keyframe bodies exceed the 128 KB reach of a conditional branch, and the long
// branches the compiler then emits inside a callee took its return-address registers.
// up to 10 free keyframes: the 8-column panel factorisation (mf_factor / mf_panel), L in Lf
template <int NF>
__device__ __forceinline__ void camera_covariance_panel(const Geometry& G, const Prob& Pr, const Work& Wk, const CovOut& O) {
    constexpr int NP = MfDims<NF>::NP, NPP = MfDims<NF>::NPP;
    __shared__ __attribute__((aligned(16))) double M[NPP * kMfLd];
    __shared__ __attribute__((aligned(16))) double Lf[NPP * kMfLd];
    __shared__ __attribute__((aligned(16))) double Up[2 * kMfPanel * kMfLd];
    __shared__ double Dv[NPP];
    __shared__ int badsh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cov_combine<kK5Threads>(G, Pr, Wk, M);
    if (tid < NPP) Dv[tid] = 0.0;
    __syncthreads();
    bool bad = false;
    if (wave == 0) mf_factor<NF, 0, true>(M, Lf, Up, lane, bad, Dv);
    __syncthreads();
    mf_panel<NF, 0, true>(M, Lf, Up, tid, bad, Dv);
    if (tid == 0) badsh = bad ? 1 : 0;
    __syncthreads();
    if (badsh) {
        if (tid == 0) O.cst[0] = -1;
        return;
    }
    cov_inverse_columns<NP, kMfLd, kK5Threads / 64>(Lf, Dv, NP, O.cc, lane, wave);
    if (tid == 0) O.cst[0] = 1;
}

// 11..20 free keyframes: the 6x6 block-pivot factorisation (bk_factor), L in place in M, the
// window padded to the template's 13 / 16 / 20 by identity rows and columns
template <int NF>
__device__ __forceinline__ void camera_covariance_blk(const Geometry& G, const Prob& Pr, const Work& Wk, const CovOut& O) {
    using D = BkDims<NF>;
    constexpr int NP = D::NP, LD = D::LD, T = 64 * kBkWaves;
    static_assert(NF > 10 && D::RPL == 2 && D::NPP <= LD, "the 11..20 free-keyframe solver");
    __shared__ __attribute__((aligned(16))) double M[16 * D::NTC * LD];
    __shared__ __attribute__((aligned(16))) double U[2 * 6 * LD];
    __shared__ __attribute__((aligned(16))) double S[72];
    __shared__ double Dv[16 * D::NTC];
    __shared__ int badsh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = 6 * G.n_free;
    cov_combine<T>(G, Pr, Wk, M);
    if (tid < 16 * D::NTC) Dv[tid] = 0.0;
    if (n < NP) {  // identity padding, as camera_solve_blk_body's
        const int np = NP - n;
        for (int e = tid; e < np * (np + 1); e += T) {
            const int c = n + e / (np + 1), r = n + e % (np + 1);
            if (r >= c) M[c * LD + r] = r == c ? 1.0 : 0.0;
        }
        for (int e = tid; e < n * np; e += T) {
            const int c = e / np, r = n + e % np;
            M[c * LD + r] = 0.0;
        }
    }
    __syncthreads();
    bool bad = false;
    bk_factor<NF, kBkWaves, true>(M, U, S, tid, bad, G.env, Dv);
    if (tid == 0) badsh = bad ? 1 : 0;
    __syncthreads();
    if (badsh) {
        if (tid == 0) O.cst[0] = -1;
        return;
    }
    cov_inverse_columns<NP, LD, kBkWaves>(M, Dv, n, O.cc, lane, wave);
    if (tid == 0) O.cst[0] = 1;
}

template <int NF>
__global__ __launch_bounds__(NF <= 10 ? kK5Threads : 64 * kBkWaves) void ba_camera_covariance(Geometry G, Prob Pr,
                                                                                                Work Wk, CovOut O) {
    if constexpr (NF <= 10)
        camera_covariance_panel<NF>(G, Pr, Wk, O);
    else
        camera_covariance_blk<NF>(G, Pr, Wk, O);
}

// Landmark covariance.  Blocks [0, n_wave): the slot waves (lane = slot): each lane forms
// Y_a = W_a V^-1 of its slot (free keyframes; zero otherwise), Z_a = sum_b Sigma_cc[a,b] Y_b over
// the landmark's lanes in slot order with Sigma_cc from global memory (L2), and the upper triangle
// of Y_a^T Z_a; the landmark's first lane sums those in slot order, adds V^-1 and stores the 9
// values and the flag.  The rest: 64 landmarks each, those without a slot (NOT_OBSERVED, zeros).
// sel: one byte per landmark (null = every landmark); a landmark not selected is only tested for
// a singular V.  Block 0 also sums the cost of x (K4's wave partials, as K5's combine does).
// bx: the block's index within its window.
__device__ __forceinline__ void landmark_covariance_body(const Geometry& G, const Prob& Pr, const Work& Wk,
                                                         const unsigned long long* obs_mask,
                                                         const unsigned char* sel, const CovOut& O, int bx) {
    __shared__ double shY[18][64];
    __shared__ double shT[6][64];
    __shared__ int shF[64];
    const int lane = threadIdx.x;
    if (bx == 0) {
        double c = 0.0;
        for (int w = lane; w < G.n_wave; w += 64) c += Wk.partA[w * kPartA];
        c = wave_sum_det(c);
        if (lane == 0) *O.cost = c;
    }
    if (bx >= G.n_wave) {
        const int l = 64 * (bx - G.n_wave) + lane;
        if (l < G.n_lm && obs_mask[l] == 0ull) {
#pragma unroll
            for (int i = 0; i < 9; ++i) O.lm[(size_t)9 * l + i] = 0.0;
            O.flags[l] = RSVIO_COV_LM_NOT_OBSERVED;
        }
        return;
    }
    const int s = 64 * bx + lane;
    const int4 h0 = Pr.slot_hdr[2 * s], h1 = Pr.slot_hdr[2 * s + 1];
    const bool act = h1.y > 0;
    const int l = h0.y, first = act ? h0.z : lane, nk = act ? h0.w : 1;
    const int fa = act ? h1.x : -1;
    const bool head = act && lane == first;
    double Vi[3][3];
    bool ok = true;
    if (act) {
        const double2* rl = reinterpret_cast<const double2*>(Wk.rawl[0] + (size_t)l * kLmF);
        double Lm[6];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double2 x = rl[i];
            Lm[2 * i] = x.x; Lm[2 * i + 1] = x.y;
        }
        ok = landmark_inverse(Lm, 0.0, Vi, 0);
    }
    if (head && !ok) atomicAdd(O.cst + 1, 1);
    const bool cam_ok = O.cst[0] == 1 || G.n_free == 0;
    bool on = act && ok && cam_ok;
    if (on && sel) on = sel[l] != 0;
    double Y[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) Y[i] = 0.0;
    if (on && fa >= 0) {
        const double2* ra = reinterpret_cast<const double2*>(Wk.raws[0] + (size_t)s * kRawF);
        double Ra[18], W[18];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const double2 x = ra[i];
            Ra[2 * i] = x.x; Ra[2 * i + 1] = x.y;
        }
        slot_w(Ra, W);
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                Y[a * 3 + k] = fma(W[a * 3 + 2], Vi[2][k], fma(W[a * 3 + 1], Vi[1][k], W[a * 3] * Vi[0][k]));
    }
#pragma unroll
    for (int i = 0; i < 18; ++i) shY[i][lane] = Y[i];
    shF[lane] = on ? fa : -1;
    __syncthreads();
    double Tq[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (on && fa >= 0) {
        const int n = 6 * G.n_free;
        double Z[18];
#pragma unroll
        for (int i = 0; i < 18; ++i) Z[i] = 0.0;
        for (int k = 0; k < nk; ++k) {
            const int fb = shF[first + k];
            if (fb < 0) continue;
            double Yb[18];
#pragma unroll
            for (int i = 0; i < 18; ++i) Yb[i] = shY[i][first + k];
            const double* Cb = O.cc + (size_t)(6 * fa) * n + 6 * fb;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double c[6];
#pragma unroll
                for (int j = 0; j < 6; ++j) c[j] = Cb[(size_t)i * n + j];
#pragma unroll
                for (int j = 0; j < 6; ++j)
#pragma unroll
                    for (int m = 0; m < 3; ++m) Z[i * 3 + m] = fma(c[j], Yb[j * 3 + m], Z[i * 3 + m]);
            }
        }
        int u = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = a; c < 3; ++c) {
                double t = 0.0;
#pragma unroll
                for (int i = 0; i < 6; ++i) t = fma(Y[i * 3 + a], Z[i * 3 + c], t);
                Tq[u++] = t;
            }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) shT[i][lane] = Tq[i];
    __syncthreads();
    if (!head || !on) return;
    double P[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < nk; ++k)
#pragma unroll
        for (int i = 0; i < 6; ++i) P[i] += shT[i][first + k];
    // V^-1 is symmetric to the last bit only in exact arithmetic: its upper triangle is taken
    P[0] += Vi[0][0]; P[1] += Vi[0][1]; P[2] += Vi[0][2];
    P[3] += Vi[1][1]; P[4] += Vi[1][2]; P[5] += Vi[2][2];
    double* o = O.lm + (size_t)9 * l;
    o[0] = P[0]; o[1] = P[1]; o[2] = P[2];
    o[3] = P[1]; o[4] = P[3]; o[5] = P[4];
    o[6] = P[2]; o[7] = P[4]; o[8] = P[5];
    O.flags[l] = RSVIO_COV_LM_OK;
}

__global__ __launch_bounds__(64) void ba_landmark_covariance(Geometry G, Prob Pr, Work Wk,
                                                             const unsigned long long* obs_mask,
                                                             const unsigned char* sel, CovOut O) {
    landmark_covariance_body(G, Pr, Wk, obs_mask, sel, O, (int)blockIdx.x);
}

// Batched mode (rsvio_ba_batch_covariance).  K4 and K4c are bab_linearize / bab_schur_chunks on a
// WinDesc table of the covariance's own views (W[2]: K4's, x as the initial state and scratch as
// the state buffers; W[0]: K4c's and the covariance kernels', x as both state buffers), G with the
// call's Huber delta, Pr the window's own with its own dense map.  Row i of the CovDesc table
// beside it holds window i's outputs and the template its single call runs (nf: n_free up to 10,
// bk_template_nf(n_free) past that, 0: no camera kernel).
struct CovDesc {
    CovOut O;
    const unsigned long long* obs_mask;
    const unsigned char* sel;
    int nf;
};

// grid B, one workgroup per window; launched once per distinct template among the active
// windows: the blocks of windows on another template return at once
template <int NF>
__global__ __launch_bounds__(NF <= 10 ? kK5Threads : 64 * kBkWaves) void bab_camera_covariance(
    const WinDesc* __restrict__ D, const CovDesc* __restrict__ Cv) {
    const WinDesc& d = D[blockIdx.x];
    const CovDesc& c = Cv[blockIdx.x];
    const int skip = d.skip, nf = c.nf;
    const Prob Pr = d.Pr;
    const Work& Wk = d.W[0];
    desc_touch(Pr.dmap, Wk.cpart);
    if (skip | (nf != NF)) return;
    if constexpr (NF <= 10)
        camera_covariance_panel<NF>(d.G, Pr, Wk, c.O);
    else
        camera_covariance_blk<NF>(d.G, Pr, Wk, c.O);
}

// grid (max over the active windows of max(n_wave + ceil(n_lm / 64), 1), B)
__global__ __launch_bounds__(64) void bab_landmark_covariance(const WinDesc* __restrict__ D,
                                                              const CovDesc* __restrict__ Cv) {
    const WinDesc& d = D[blockIdx.y];
    const CovDesc& c = Cv[blockIdx.y];
    const int skip = d.skip, bound = max(d.G.n_wave + (d.G.n_lm + 63) / 64, 1);
    const Prob Pr = d.Pr;
    const Work& Wk = d.W[0];
    const unsigned long long* obs_mask = c.obs_mask;
    desc_touch(Pr.slot_hdr, Wk.rawl[0], Wk.partA, obs_mask);
    if (skip | ((int)blockIdx.x >= bound)) return;
    landmark_covariance_body(d.G, Pr, Wk, obs_mask, c.sel, c.O, (int)blockIdx.x);
}
