"""Motion tracking (PnP) + keyframe rule over the C ABI (rsvio_pnp_*, rsvio_track_motion*).

Mirrors SlidingWindow::track_motion (src/estimator/sliding_window.rs:490-587) and the
keyframe decision of Estimator::process_frame (src/estimator/estimator.rs:195-234): one
device launch per frame runs the map join, the PnP LM (10 iterations, Huber 2.0), the
success test, T_W_B = inv(SE3) and the translation / euler-angle thresholds.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import check, ptr


def pnp_cfg(max_iterations=10, cost_tolerance=1e-6, parameter_tolerance=1e-9, huber_delta=2.0, lambda_init=1e-4):
    """sliding_window.rs:494-501 (SparseCholesky; + HuberLoss::new(2.0) at :538)."""
    return _lib.LmCfg(max_iterations, cost_tolerance, parameter_tolerance, huber_delta, lambda_init, 1)


@dataclass
class MotionResult:
    status: int
    iterations: int
    is_keyframe: bool
    n_observations: int
    initial_cost: float
    final_cost: float
    translation_norm: float
    rotation_norm: float
    T_W_B: np.ndarray
    kernel_ms: float = 0.0  # device time of the launch (wall clock; no host or copy time)

    @property
    def success(self) -> bool:
        """is_optimization_successful (sliding_window.rs:384-395)."""
        return self.status > 0


def _result(r: _lib.MotionResult) -> MotionResult:
    return MotionResult(r.status, r.iterations, bool(r.is_keyframe), r.n_observations, r.initial_cost, r.final_cost,
                        r.translation_norm, r.rotation_norm, np.array(r.T_W_B[:], np.float64).reshape(4, 4),
                        r.kernel_ms)


@dataclass
class RansacConfig:
    """rsvio_ransac_cfg: n_hyp hypotheses (h = 0 the prior), the seed of the pair sampler, the
    inlier test (squared normalised reprojection error: 1e-4 is about 4.6 px at EuRoC's fx; depth
    along the optical axis: the reference configs' 0.1 m) and the smallest consensus accepted."""
    n_hyp: int = 256
    min_inliers: int = 10
    seed: int = 0
    inlier_sq_error: float = 1e-4
    min_depth: float = 0.1

    def to_c(self) -> _lib.RansacCfg:
        return _lib.RansacCfg(int(self.n_hyp), int(self.min_inliers), int(self.seed) & (2 ** 64 - 1),
                              float(self.inlier_sq_error), float(self.min_depth))


RANSAC_OK, RANSAC_TOO_FEW_PAIRS, RANSAC_NO_CONSENSUS = 1, 2, -1


@dataclass
class RobustMotionResult:
    """rsvio_robust_motion_result plus the masks (0 no map point, 1 inlier, 2 outlier, indexed like
    the feature lists) and, on request, the inlier count of every hypothesis (-1: invalid)."""
    motion: MotionResult
    ransac_status: int
    n_pairs: int
    n_valid_pairs: int
    n_valid_hyp: int
    best_hyp: int
    best_count: int
    n_inliers: int
    device_ms: float
    mask_l: np.ndarray
    mask_r: np.ndarray
    hyp_count: np.ndarray | None = None


def _samples(samples, n_hyp):
    if samples is None:
        return None
    samples = np.ascontiguousarray(samples, np.int32)
    if samples.shape != (n_hyp, 3):
        raise ValueError(f"samples must be n_hyp x 3 = ({n_hyp}, 3), got {samples.shape}")
    return samples


def _robust_result(r: _lib.RobustMotionResult, mask_l, mask_r, counts) -> RobustMotionResult:
    return RobustMotionResult(_result(r.motion), r.ransac_status, r.n_pairs, r.n_valid_pairs, r.n_valid_hyp,
                              r.best_hyp, r.best_count, r.n_inliers, r.device_ms, mask_l, mask_r, counts)


MCOV_OK, MCOV_TOO_FEW, MCOV_SINGULAR = 1, -1, -2


@dataclass
class PoseCovariance:
    """rsvio_motion_covariance's outcome: cov = H^-1 of the PnP Hessian H = sum w J^T J at
    T_B_W = inverse(T_W_B), in the LM's tangent (T_B_W <- T_B_W Exp([dt; dw])) -- equally the
    covariance of T_W_B under the left perturbation Exp(-d) T_W_B -- per unit measurement variance
    in normalised image units^2.  All NaN unless status is MCOV_OK (MCOV_TOO_FEW: fewer than 3
    factors; MCOV_SINGULAR: a pivot of H not positive and finite)."""
    status: int
    cov: np.ndarray           # 6 x 6, symmetric bit for bit
    n_observations: int       # factors used
    n_downweighted: int       # ... with a Huber weight below 1
    cost: float               # sum rho / 2 over the factors (MotionResult.final_cost's definition)
    min_pivot: float          # smallest LDL^T pivot (0: not factorised)
    kernel_ms: float

    @property
    def ok(self) -> bool:
        return self.status == MCOV_OK


def _pose_cov(cov, i: _lib.MotionCovInfo) -> PoseCovariance:
    return PoseCovariance(i.status, np.array(cov, np.float64).reshape(6, 6), i.n_observations, i.n_downweighted,
                          i.cost, i.min_pivot, i.kernel_ms)


def _mask(mask, n, what):
    if mask is None:
        return None
    mask = np.ascontiguousarray(mask, np.uint8).reshape(-1)
    if len(mask) != n:
        raise ValueError(f"{what} has {len(mask)} bytes for {n} features")
    return mask


class MotionTracker:
    """Device handle for track_motion; holds the map (ids ascending, p_W as f32)."""

    def __init__(self, device: int = 0, translation_threshold: float = 0.05, rotation_threshold: float = 0.05):
        h = C.c_void_p()
        check(_lib.load().rsvio_pnp_create(device, C.byref(h)))
        self._h = h
        self.rule = _lib.KeyframeRule(translation_threshold, rotation_threshold)
        self.n_map = 0

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().rsvio_pnp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        """Launch on a caller-owned HIP stream (None: the handle's own)."""
        check(_lib.load().rsvio_pnp_set_stream(self._h, stream_ptr))

    def set_map(self, ids, p_W):
        """map_points (sliding_window.rs:466-475); sorted here if the caller's ids are not."""
        ids = np.asarray(ids, np.uint64).reshape(-1)
        p_W = np.asarray(p_W, np.float32).reshape(-1, 3)
        order = np.argsort(ids, kind="stable")
        ids = np.ascontiguousarray(ids[order])
        p_W = np.ascontiguousarray(p_W[order])
        check(_lib.load().rsvio_pnp_set_map(self._h, ptr(ids), ptr(p_W), len(ids)))
        self.n_map = len(ids)

    def map_stats(self) -> dict:
        """Diagnostic (rsvio_dbg_pnp_map_stats): the hash table the last set_map built --
        buckets, max_probe (the longest bucket run an insertion took), has_top (the id 2^64 - 1 is
        in the map, carried beside the table) and n_map."""
        fn = _lib.load().rsvio_dbg_pnp_map_stats
        fn.argtypes = [C.c_void_p, C.c_void_p]
        fn.restype = C.c_int
        out = np.zeros(4, np.int32)
        check(fn(self._h, ptr(out)))
        return dict(buckets=int(out[0]), max_probe=int(out[1]), has_top=int(out[2]), n_map=int(out[3]))

    def track_motion(self, ids_l, uv_l, ids_r, uv_r, T_W_B_last_kf, T_C_B2, cfg=None) -> MotionResult:
        ids_l = np.ascontiguousarray(ids_l, np.uint64).reshape(-1)
        ids_r = np.ascontiguousarray(ids_r, np.uint64).reshape(-1)
        uv_l = np.ascontiguousarray(uv_l, np.float32).reshape(-1, 2)
        uv_r = np.ascontiguousarray(uv_r, np.float32).reshape(-1, 2)
        Tl = np.ascontiguousarray(T_W_B_last_kf, np.float64).reshape(16)
        tcb = np.ascontiguousarray(T_C_B2, np.float64).reshape(32)
        cfg = cfg or pnp_cfg()
        r = _lib.MotionResult()
        check(_lib.load().rsvio_track_motion(self._h, ptr(ids_l), ptr(uv_l), len(ids_l), ptr(ids_r), ptr(uv_r),
                                             len(ids_r), ptr(Tl), ptr(tcb), C.byref(cfg), C.byref(self.rule),
                                             C.byref(r)))
        return _result(r)

    def track_motion_tracker(self, tracker, T_W_B_last_kf, T_C_B2, cfg=None) -> MotionResult:
        """Features of the tracker's last frame, read on the device (no host round trip)."""
        Tl = np.ascontiguousarray(T_W_B_last_kf, np.float64).reshape(16)
        tcb = np.ascontiguousarray(T_C_B2, np.float64).reshape(32)
        cfg = cfg or pnp_cfg()
        r = _lib.MotionResult()
        check(_lib.load().rsvio_track_motion_tracker(self._h, tracker._h, ptr(Tl), ptr(tcb), C.byref(cfg),
                                                     C.byref(self.rule), C.byref(r)))
        return _result(r)

    def track_motion_robust(self, ids_l, uv_l, ids_r, uv_r, T_W_B_last_kf, T_C_B2, ransac: RansacConfig | None = None,
                            cfg=None, samples=None, want_counts: bool = False) -> RobustMotionResult:
        """track_motion behind a stereo 3-point RANSAC (rsvio_track_motion_robust): hypotheses from
        `samples` (n_hyp x 3 pair indices) or the seeded sampler, the LM on the winner's inliers."""
        ids_l = np.ascontiguousarray(ids_l, np.uint64).reshape(-1)
        ids_r = np.ascontiguousarray(ids_r, np.uint64).reshape(-1)
        uv_l = np.ascontiguousarray(uv_l, np.float32).reshape(-1, 2)
        uv_r = np.ascontiguousarray(uv_r, np.float32).reshape(-1, 2)
        Tl = np.ascontiguousarray(T_W_B_last_kf, np.float64).reshape(16)
        tcb = np.ascontiguousarray(T_C_B2, np.float64).reshape(32)
        cfg = cfg or pnp_cfg()
        rc = (ransac or RansacConfig()).to_c()
        samples = _samples(samples, rc.n_hyp)
        mask_l, mask_r = np.zeros(len(ids_l), np.uint8), np.zeros(len(ids_r), np.uint8)
        counts = np.zeros(max(rc.n_hyp, 0), np.int32) if want_counts else None
        r = _lib.RobustMotionResult()
        check(_lib.load().rsvio_track_motion_robust(self._h, ptr(ids_l), ptr(uv_l), len(ids_l), ptr(ids_r), ptr(uv_r),
                                                    len(ids_r), ptr(Tl), ptr(tcb), C.byref(cfg), C.byref(self.rule),
                                                    C.byref(rc), ptr(samples), ptr(mask_l), ptr(mask_r), ptr(counts),
                                                    C.byref(r)))
        return _robust_result(r, mask_l, mask_r, counts)

    def track_motion_tracker_robust(self, tracker, T_W_B_last_kf, T_C_B2, ransac: RansacConfig | None = None,
                                    cfg=None, samples=None, want_counts: bool = False) -> RobustMotionResult:
        """The robust call on the tracker's last collected frame, read on the device; the masks
        are indexed like the collected feature lists."""
        Tl = np.ascontiguousarray(T_W_B_last_kf, np.float64).reshape(16)
        tcb = np.ascontiguousarray(T_C_B2, np.float64).reshape(32)
        cfg = cfg or pnp_cfg()
        rc = (ransac or RansacConfig()).to_c()
        samples = _samples(samples, rc.n_hyp)
        # the library writes as many bytes as the collected frame has features: buffers of the
        # tracker's capacity, cut to the collected lists' lengths
        n_l, n_r = tracker._n
        mask_l, mask_r = np.zeros(max(tracker.cap, n_l), np.uint8), np.zeros(max(tracker.cap, n_r), np.uint8)
        counts = np.zeros(max(rc.n_hyp, 0), np.int32) if want_counts else None
        r = _lib.RobustMotionResult()
        check(_lib.load().rsvio_track_motion_robust_tracker(self._h, tracker._h, ptr(Tl), ptr(tcb), C.byref(cfg),
                                                            C.byref(self.rule), C.byref(rc), ptr(samples),
                                                            ptr(mask_l), ptr(mask_r), ptr(counts), C.byref(r)))
        return _robust_result(r, mask_l[:n_l].copy(), mask_r[:n_r].copy(), counts)

    def covariance(self, ids_l, uv_l, ids_r, uv_r, T_W_B, T_C_B2, huber_delta: float = 2.0, mask_l=None,
                   mask_r=None) -> PoseCovariance:
        """The 6x6 covariance of the pose T_W_B given these features and the handle's map
        (rsvio_motion_covariance).  mask_l / mask_r: one byte per feature, 1 = use (the masks
        track_motion_robust returns); None: every feature with a map point."""
        ids_l = np.ascontiguousarray(ids_l, np.uint64).reshape(-1)
        ids_r = np.ascontiguousarray(ids_r, np.uint64).reshape(-1)
        uv_l = np.ascontiguousarray(uv_l, np.float32).reshape(-1, 2)
        uv_r = np.ascontiguousarray(uv_r, np.float32).reshape(-1, 2)
        mask_l, mask_r = _mask(mask_l, len(ids_l), "mask_l"), _mask(mask_r, len(ids_r), "mask_r")
        T = np.ascontiguousarray(T_W_B, np.float64).reshape(16)
        tcb = np.ascontiguousarray(T_C_B2, np.float64).reshape(32)
        cov, info = np.empty(36, np.float64), _lib.MotionCovInfo()
        check(_lib.load().rsvio_motion_covariance(self._h, ptr(ids_l), ptr(uv_l), len(ids_l), ptr(ids_r), ptr(uv_r),
                                                  len(ids_r), ptr(mask_l), ptr(mask_r), ptr(T), ptr(tcb),
                                                  float(huber_delta), ptr(cov), C.byref(info)))
        return _pose_cov(cov, info)

    def covariance_tracker(self, tracker, T_W_B, T_C_B2, huber_delta: float = 2.0, mask_l=None,
                           mask_r=None) -> PoseCovariance:
        """covariance() on the tracker's last collected frame, read on the device; the masks are
        host arrays indexed like the collected feature lists."""
        n_l, n_r = tracker._n
        mask_l, mask_r = _mask(mask_l, n_l, "mask_l"), _mask(mask_r, n_r, "mask_r")
        T = np.ascontiguousarray(T_W_B, np.float64).reshape(16)
        tcb = np.ascontiguousarray(T_C_B2, np.float64).reshape(32)
        cov, info = np.empty(36, np.float64), _lib.MotionCovInfo()
        check(_lib.load().rsvio_motion_covariance_tracker(self._h, tracker._h, ptr(mask_l), ptr(mask_r), ptr(T),
                                                          ptr(tcb), float(huber_delta), ptr(cov), C.byref(info)))
        return _pose_cov(cov, info)


@dataclass
class MotionFrame:
    """One slot's frame of a MotionBatch run (rsvio_motion_frame).  Host arrays, or -- with
    `on_device` -- lists already on the device, read in place: `ids_l` / `ids_r` torch uint8 device
    buffers holding the u64 ids `id_stride` bytes apart (0: 8; sizeof(rsvio_feature) for tracker
    output), with `n_l` / `n_r` ids in them, and `uv_l` / `uv_r` float32 (n, 2) device tensors -- or
    all four as device addresses (ints, e.g. StereoPatchTracker.device_lists()) with `n_l` / `n_r`."""
    ids_l: object
    uv_l: object
    ids_r: object
    uv_r: object
    T_W_B_last_kf: np.ndarray
    T_C_B2: np.ndarray
    cfg: object = None        # this slot's LM cfg (None: the call's)
    samples: object = None    # robust only: n_hyp x 3 pair indices (None: the seeded sampler)
    on_device: bool = False
    id_stride: int = 0
    n_l: int | None = None    # on_device: the number of ids (None: len(uv_l))
    n_r: int | None = None


def _device_list(ids, uv, n, stride):
    """(ids pointer, uv pointer, n) of a device-resident list; the tensors must outlive the run."""
    import torch
    if n is None and isinstance(uv, int):
        raise ValueError("on_device lists given as addresses need n_l / n_r")
    n = len(uv) if n is None else int(n)
    if n == 0:
        return None, None, 0
    if isinstance(ids, int) and isinstance(uv, int):   # raw device addresses (StereoPatchTracker.device_lists)
        return ids, uv, n
    if not (isinstance(ids, torch.Tensor) and ids.is_cuda and ids.dtype == torch.uint8 and ids.is_contiguous()):
        raise ValueError("on_device ids must be a contiguous torch uint8 device buffer")
    if not (isinstance(uv, torch.Tensor) and uv.is_cuda and uv.dtype == torch.float32 and uv.is_contiguous() and
            tuple(uv.shape) == (n, 2)):
        raise ValueError("on_device uv must be a contiguous float32 (n, 2) device tensor")
    if ids.numel() < (n - 1) * (stride or 8) + 8:
        raise ValueError("on_device ids buffer is shorter than n ids at id_stride")
    return ids.data_ptr(), uv.data_ptr(), n


class MotionBatch:
    """rsvio_pnp_batch: one frame per MotionTracker -- each with its own map -- tracked by one launch
    (plain) or three (robust) with one upload and one host wait; every result is bit for bit the
    tracker's own track_motion / track_motion_robust result.  The trackers are borrowed (they must
    outlive the batch; the same one may sit in several slots); slot i uses trackers[i]'s current
    map and the FIRST tracker's keyframe rule."""

    def __init__(self, trackers):
        self.trackers = list(trackers)
        self.n = len(self.trackers)
        arr = (C.c_void_p * max(self.n, 1))(*[t._h.value for t in self.trackers])
        h = C.c_void_p()
        check(_lib.load().rsvio_pnp_batch_create(arr, self.n, C.byref(h)))
        self._h = h
        self.rule = self.trackers[0].rule
        self.device_ms = 0.0   # of the last run: the batch's launches by HIP events

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().rsvio_pnp_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _frames(self, frames, n_hyp=None):
        """The ctypes frame table and the arrays it points into (kept alive by the caller)."""
        if len(frames) != self.n:
            raise ValueError(f"{len(frames)} frames for a batch of {self.n}")
        tab = (_lib.MotionFrame * self.n)()
        keep = []
        for i, f in enumerate(frames):
            c = tab[i]
            if f.on_device:
                c.ids_l, c.uv_l, c.n_l = _device_list(f.ids_l, f.uv_l, f.n_l, f.id_stride)
                c.ids_r, c.uv_r, c.n_r = _device_list(f.ids_r, f.uv_r, f.n_r, f.id_stride)
                c.on_device, c.id_stride = 1, int(f.id_stride)
                keep.append((f.ids_l, f.uv_l, f.ids_r, f.uv_r))
            else:
                ids_l = np.ascontiguousarray(f.ids_l, np.uint64).reshape(-1)
                ids_r = np.ascontiguousarray(f.ids_r, np.uint64).reshape(-1)
                uv_l = np.ascontiguousarray(f.uv_l, np.float32).reshape(-1, 2)
                uv_r = np.ascontiguousarray(f.uv_r, np.float32).reshape(-1, 2)
                if len(uv_l) != len(ids_l) or len(uv_r) != len(ids_r):
                    raise ValueError(f"slot {i}: ids and uv differ in length")
                c.ids_l, c.uv_l, c.n_l = ptr(ids_l), ptr(uv_l), len(ids_l)
                c.ids_r, c.uv_r, c.n_r = ptr(ids_r), ptr(uv_r), len(ids_r)
                keep.append((ids_l, uv_l, ids_r, uv_r))
            # (None: left NULL -- the covariance call does not read it, the tracking calls refuse)
            Tl = None if f.T_W_B_last_kf is None else np.ascontiguousarray(f.T_W_B_last_kf, np.float64).reshape(16)
            tcb = np.ascontiguousarray(f.T_C_B2, np.float64).reshape(32)
            c.T_W_B_last_kf, c.T_C_B2 = ptr(Tl), ptr(tcb)
            keep.append((Tl, tcb, f.cfg))
            if f.cfg is not None:
                c.cfg = C.pointer(f.cfg)
            if n_hyp is not None and f.samples is not None:
                smp = _samples(f.samples, n_hyp)
                c.samples = ptr(smp)
                keep.append(smp)
        return tab, keep

    def track_motion(self, frames, cfg=None) -> list[MotionResult]:
        cfg = cfg or pnp_cfg()
        tab, keep = self._frames(frames)
        res = (_lib.MotionResult * self.n)()
        ms = C.c_double(0.0)
        check(_lib.load().rsvio_pnp_batch_track_motion(self._h, C.addressof(tab), C.byref(cfg), C.byref(self.rule),
                                                       C.addressof(res), C.byref(ms)))
        del keep
        self.device_ms = ms.value
        return [_result(r) for r in res]

    def track_motion_robust(self, frames, ransac: RansacConfig | None = None, cfg=None,
                            want_counts: bool = False, want_masks: bool = True) -> list[RobustMotionResult]:
        """want_counts / want_masks: one bool, or one per slot; a slot without leaves its pointers
        NULL (hyp_count, mask_l / mask_r come back None)."""
        cfg = cfg or pnp_cfg()
        rc = (ransac or RansacConfig()).to_c()
        tab, keep = self._frames(frames, n_hyp=rc.n_hyp)
        wm = [want_masks] * self.n if isinstance(want_masks, bool) else list(want_masks)
        wc = [want_counts] * self.n if isinstance(want_counts, bool) else list(want_counts)
        outs = []
        for i in range(self.n):
            c = tab[i]
            ml = np.zeros(c.n_l, np.uint8) if wm[i] else None
            mr = np.zeros(c.n_r, np.uint8) if wm[i] else None
            cnt = np.zeros(max(rc.n_hyp, 0), np.int32) if wc[i] else None
            c.mask_l, c.mask_r, c.hyp_count = ptr(ml), ptr(mr), ptr(cnt)
            outs.append((ml, mr, cnt))
        res = (_lib.RobustMotionResult * self.n)()
        ms = C.c_double(0.0)
        check(_lib.load().rsvio_pnp_batch_track_motion_robust(self._h, C.addressof(tab), C.byref(cfg),
                                                              C.byref(self.rule), C.byref(rc), C.addressof(res),
                                                              C.byref(ms)))
        del keep
        self.device_ms = ms.value
        return [_robust_result(r, *o) for r, o in zip(res, outs)]

    def covariance(self, frames, T_W_B, huber_delta: float = 2.0, masks=None) -> list[PoseCovariance]:
        """Slot i's pose covariance at T_W_B[i] (n x 4 x 4) for frames[i] on trackers[i]'s map, all
        in one launch (rsvio_pnp_batch_covariance); each bit for bit the tracker's own covariance().
        Of a frame only the lists and T_C_B2 are read.  masks: None, or per slot None or
        (mask_l, mask_r) -- host arrays, each of which may be None."""
        tab, keep = self._frames(frames)
        T = np.ascontiguousarray(T_W_B, np.float64).reshape(self.n, 16)
        if masks is not None:
            if len(masks) != self.n:
                raise ValueError(f"{len(masks)} masks for a batch of {self.n}")
            for i, m in enumerate(masks):
                if m is None:
                    continue
                ml = _mask(m[0], tab[i].n_l, f"slot {i}: mask_l")
                mr = _mask(m[1], tab[i].n_r, f"slot {i}: mask_r")
                tab[i].mask_l, tab[i].mask_r = ptr(ml), ptr(mr)
                keep.append((ml, mr))
        cov = np.empty((self.n, 36), np.float64)
        info = (_lib.MotionCovInfo * self.n)()
        ms = C.c_double(0.0)
        check(_lib.load().rsvio_pnp_batch_covariance(self._h, C.addressof(tab), ptr(T), float(huber_delta), ptr(cov),
                                                     C.addressof(info), C.byref(ms)))
        del keep
        self.device_ms = ms.value
        return [_pose_cov(cov[i], info[i]) for i in range(self.n)]
