"""CPU reference of motion-predicted tracking (include/rsvio_gpu.h, rsvio_tracker_set_prediction),
put together from what the oracle library already exports.

  predict_seeds(cam, R, px, w, h)   oracle.unproject -> the bearing and rotation in numpy f64, every sum
                                    written out left to right -> oracle.project -> f32 -> the in-image rule
  track_one_seeded(...)             track_one_point (tracker_oracle.cpp) with the search started at a seed:
                                    orc_track_point_at_level per level, coarse to fine, levels sliced with
                                    orc_pyramid_offset, then mat3_mul(T0, T1)'s 2 x 2 in f32
  track_points_seeded(...)          forward from the seed, backward from the inverse prediction
                                    bs = fwd.t - (seed - T0.t), the 0.4 test in f32
fixture(theta) is rsvio.synthetic.rotating_scene_pair's left camera as the tests use it: both pyramids,
the features oracle.detect_key_points finds in frame 0 as identity affines, and the OPENCV5 PLANE camera.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from oracle import oracle as O

W, H, LEVELS, GRID = 376, 240, 3, 30
f32 = np.float32


def _at_level():
    lib = O.load()
    fn = lib.orc_track_point_at_level
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_float]
    return fn


def level(pyr: np.ndarray, w: int, h: int, i: int) -> np.ndarray:
    off = int(O.load().orc_pyramid_offset(w, h, i))
    lw, lh = w >> i, h >> i
    return np.ascontiguousarray(pyr[off:off + lw * lh])


def track_one_seeded(pyr0, pyr1, w, h, levels, T0, seed, max_it, thresh):
    """T0: 6 f32 {m00, m01, m10, m11, tx, ty}; seed: 2 f32.  (ok, 6 f32 result)."""
    fn = _at_level()
    T0 = np.asarray(T0, f32)
    T1 = np.array([1, 0, 0, 1, seed[0], seed[1]], f32)
    for i in range(levels - 1, -1, -1):
        sdn = f32(1 << i)
        T1[4] = T1[4] / sdn
        T1[5] = T1[5] / sdn
        l0, l1 = level(pyr0, w, h, i), level(pyr1, w, h, i)
        ok = fn(l1.ctypes.data, w >> i, h >> i, l0.ctypes.data, C.c_float(T0[4] / sdn), C.c_float(T0[5] / sdn),
                T1.ctypes.data, max_it, C.c_float(thresh))
        if not ok:
            return False, None
        T1[4] = T1[4] * sdn
        T1[5] = T1[5] * sdn
    # mat3_mul(T0, T1) (tracker_oracle.cpp): acc = a_i0 b_0j; acc = a_i1 b_1j + acc; acc = a_i2 b_2j + acc, f32
    A = np.array([[T0[0], T0[1], T0[4]], [T0[2], T0[3], T0[5]], [0, 0, 1]], f32)
    B = np.array([[T1[0], T1[1], T1[4]], [T1[2], T1[3], T1[5]], [0, 0, 1]], f32)
    out = T1.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(2):
            for j in range(2):
                acc = f32(A[i, 0] * B[0, j])
                acc = f32(f32(A[i, 1] * B[1, j]) + acc)
                acc = f32(f32(A[i, 2] * B[2, j]) + acc)
                out[2 * i + j] = acc
    return True, out


def track_points_seeded(pyr0, pyr1, w, h, levels, aff, seeds, max_it=20, thresh=0.01):
    """(aff_out n x 6 f32, valid bool): rsvio_track_points_seeded's contract."""
    aff = np.ascontiguousarray(aff, f32).reshape(-1, 6)
    seeds = np.ascontiguousarray(seeds, f32).reshape(-1, 2)
    out, valid = aff.copy(), np.zeros(len(aff), bool)
    for k, (T0, s) in enumerate(zip(aff, seeds)):
        s = s.copy() if np.all(np.isfinite(s)) else T0[4:6].copy()   # a non-finite seed: the own position
        ok, fwd = track_one_seeded(pyr0, pyr1, w, h, levels, T0, s, max_it, thresh)
        if not ok:
            continue
        bs = np.array([fwd[4] - f32(s[0] - T0[4]), fwd[5] - f32(s[1] - T0[5])], f32)
        ok, bwd = track_one_seeded(pyr1, pyr0, w, h, levels, fwd, bs, max_it, thresh)
        if not ok:
            continue
        dx, dy = f32(T0[4] - bwd[4]), f32(T0[5] - bwd[5])
        if f32(f32(dx * dx) + f32(dy * dy)) < f32(0.4):
            out[k], valid[k] = fwd, True
    return out, valid


def predict_seeds(cam: O.OrcCamera, R, px, w, h):
    """(seeds n x 2 f32, seeded bool): rsvio_predict_seeds' contract; R = R_cur_prev, 3 x 3."""
    px = np.ascontiguousarray(px, f32).reshape(-1, 2)
    R = np.asarray(R, np.float64).reshape(3, 3)
    und, ok = O.unproject(cam, px)
    x, y = und[:, 0].astype(np.float64), und[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        z = np.sqrt(np.maximum(0.0, (1.0 - x * x) - y * y)) if cam.convention == 1 else np.ones_like(x)
        q = np.stack([(R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z for i in range(3)], 1)
    uv, valid = O.project(cam, np.ascontiguousarray(q))   # (a NaN bearing fails its Z > 0 / den > 0 test)
    uv = uv.astype(f32)
    with np.errstate(invalid="ignore"):
        seeded = (ok & valid & np.isfinite(uv).all(1) & (uv[:, 0] >= 0) & (uv[:, 0] <= f32(w - 1)) & (uv[:, 1] >= 0) &
                  (uv[:, 1] <= f32(h - 1)))
    return np.where(seeded[:, None], uv, px).astype(f32), seeded


def opencv5_camera(intr, convention: int = 0) -> O.OrcCamera:
    """OPENCV5 with a stream's radtan parameters (fx, fy, cx, cy, k1, k2, p1, p2) and k3 = 0."""
    return O.camera(0, list(intr[:8]) + [0.0], convention)


def rsvio_camera(cam: O.OrcCamera):
    """The same camera for the product library."""
    from rsvio.camera import Camera
    n = 6 if cam.model == 1 else 9
    return Camera(cam.model, [cam.params[i] for i in range(n)], "ray" if cam.convention == 1 else "plane",
                  cam.max_iterations)


@functools.lru_cache(maxsize=None)
def scene_pair(theta_deg: float, w: int = W, h: int = H):
    """rotating_scene_pair, rendered once per argument set (treat as read-only)."""
    from rsvio import synthetic as S
    return S.rotating_scene_pair(theta_deg, w, h)


@functools.lru_cache(maxsize=None)
def fixture(theta_deg: float, cam_index: int = 0, levels: int = LEVELS, w: int = W, h: int = H, grid: int = GRID):
    """(pyr0, pyr1, aff n x 6, camera, R hint, pair) of rotating_scene_pair(theta) for one camera;
    computed once per argument set and shared (treat as read-only)."""
    pair = scene_pair(theta_deg, w, h)
    img0, img1 = pair.frames[0][cam_index], pair.frames[1][cam_index]
    pyr0, pyr1 = O.build_pyramid(img0, levels), O.build_pyramid(img1, levels)
    pts, _ = O.detect_key_points(img0, grid)
    aff = np.zeros((len(pts), 6), f32)
    aff[:, 0] = aff[:, 3] = 1.0
    aff[:, 4:6] = pts.astype(f32)
    for a in (pyr0, pyr1, aff):
        a.setflags(write=False)
    return pyr0, pyr1, aff, opencv5_camera(pair.intrinsics[cam_index]), pair.R_cur_prev, pair
