// tracker_predict.hpp -- motion-predicted tracking: where a feature's bearing lands after a rotation
// hint (an integrated gyro, or the last inter-frame rotation), as the start of its LK search.  Part
// of tracker.hip's translation unit.
//
// The contract is include/rsvio_gpu.h's (rsvio_predict_seeds, rsvio_tracker_set_prediction).  For a
// feature at pixel (u, v) of a camera:
//   (x, y, ok) = unproject_one(cam, u, v)          the f32 values the fused unprojection stores
//   b          = (x, y, 1) (PLANE) or (x, y, sqrt(max(0, (1 - x x) - y y))) (RAY), f64
//   q          = R b                               row-major, each row summed left to right
//   (u', v')   = project_one(cam, q)               narrowed to f32
// seeded iff ok, the projection is valid, both values are finite, 0 <= u' <= w - 1 and
// 0 <= v' <= h - 1; otherwise the seed is (u, v) itself and the feature counts as unseeded.
#pragma once

// One launch covers both cameras: thread j < n[0] is entry j of camera 0, the rest camera 1's.
struct PredictArgs {
    rsvio_camera cam[2];
    double R[2][9];        // R_cur_prev per camera, row-major
    const float* pos[2];   // entry i's pixel at pos[c][stride * i + off], + 1
    float2* seeds[2];
    uint8_t* seeded[2];
    int n[2];
    int stride, off;       // 2, 0: pixel pairs; 6, 4: the track maps' affines
    int w, h;
};

__global__ __launch_bounds__(256) void predict_seeds_kernel(PredictArgs A) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= A.n[0] + A.n[1]) return;
    const int c = j < A.n[0] ? 0 : 1;
    const int i = c == 0 ? j : j - A.n[0];
    const float* p = A.pos[c] + (size_t)A.stride * i + A.off;
    const float u = p[0], v = p[1];
    const rsvio_camera& cam = A.cam[c];
    const Undist un = unproject_one(cam, u, v);
    const double x = (double)un.x, y = (double)un.y;
    const double z = cam.convention == RSVIO_UNPROJ_RAY ? sqrt(fmax(0.0, (1.0 - x * x) - y * y)) : 1.0;
    const double* R = A.R[c];
    const double qx = (R[0] * x + R[1] * y) + R[2] * z;
    const double qy = (R[3] * x + R[4] * y) + R[5] * z;
    const double qz = (R[6] * x + R[7] * y) + R[8] * z;
    const Proj pr = project_one(cam, qx, qy, qz);
    const float su = (float)pr.u, sv = (float)pr.v;
    const bool ok = un.ok && pr.ok && isfinite(su) && isfinite(sv) && su >= 0.0f && su <= (float)(A.w - 1) &&
                    sv >= 0.0f && sv <= (float)(A.h - 1);
    A.seeds[c][i] = ok ? make_float2(su, sv) : make_float2(u, v);
    A.seeded[c][i] = ok ? 1 : 0;
}
