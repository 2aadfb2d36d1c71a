"""Host-side mirror of the reference tracker API over the C ABI.

``StereoPatchTracker`` mirrors ``StereoPatchTracker<LEVELS>``
(src/feature_tracker/feature_tracker.rs:91-207): ``new(grid_size, max_iters, thresh)``,
``process_frame(left, right)``, ``get_track_points()``, ``remove_id(ids)``.  The free
functions mirror the reference's module-level ``build_image_pyramid`` (:209-220),
``track_points`` (:252-291) and ``image_utilities::detect_key_points`` (:108-175).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import check, ptr


def pyramid_bytes(w: int, h: int, levels: int) -> int:
    return int(_lib.load().rsvio_pyramid_bytes(w, h, levels))


def pyramid_levels(pyr: np.ndarray, w: int, h: int, levels: int) -> list[np.ndarray]:
    out, off = [], 0
    for i in range(levels):
        lw, lh = w // (1 << i), h // (1 << i)
        out.append(pyr[off:off + lw * lh].reshape(lh, lw))
        off += lw * lh
    return out


def build_image_pyramid(img: np.ndarray, levels: int) -> np.ndarray:
    """Packed u8 pyramid (level 0 first) of a u8 H x W image."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    out = np.empty(pyramid_bytes(w, h, levels), np.uint8)
    check(_lib.load().rsvio_build_pyramid(ptr(img), w, h, levels, ptr(out)))
    return out


def track_points(pyr0: np.ndarray, pyr1: np.ndarray, w: int, h: int, levels: int, aff: np.ndarray,
                 max_iterations: int = 20, thresh: float = 0.01):
    """Forward/backward tracking of n Affine2 states (n x 6 f32); returns (aff_out, valid)."""
    aff = np.ascontiguousarray(aff, np.float32).reshape(-1, 6)
    n = aff.shape[0]
    out = np.empty_like(aff)
    valid = np.zeros(n, np.uint8)
    check(_lib.load().rsvio_track_points(ptr(pyr0), ptr(pyr1), w, h, levels, ptr(aff), n, max_iterations,
                                         C.c_float(thresh), ptr(out), ptr(valid)))
    return out, valid.astype(bool)


def track_points_seeded(pyr0: np.ndarray, pyr1: np.ndarray, w: int, h: int, levels: int, aff: np.ndarray,
                        seeds: np.ndarray, max_iterations: int = 20, thresh: float = 0.01):
    """rsvio_track_points_seeded: track_points with feature i's search started at seeds[i] (n x 2 f32
    pixels of the second image; a non-finite seed: its own position); returns (aff_out, valid)."""
    aff = np.ascontiguousarray(aff, np.float32).reshape(-1, 6)
    seeds = np.ascontiguousarray(seeds, np.float32).reshape(-1, 2)
    n = aff.shape[0]
    if len(seeds) != n:
        raise ValueError("one seed per feature")
    out = np.empty_like(aff)
    valid = np.zeros(n, np.uint8)
    check(_lib.load().rsvio_track_points_seeded(ptr(pyr0), ptr(pyr1), w, h, levels, ptr(aff), ptr(seeds), n,
                                                max_iterations, C.c_float(thresh), ptr(out), ptr(valid)))
    return out, valid.astype(bool)


def predict_seeds(camera, R, px, w: int, h: int):
    """rsvio_predict_seeds: where the bearings of n pixels (n x 2 f32) of `camera` (rsvio.camera.Camera)
    land after the rotation R = R_cur_prev (3 x 3), as pixels of a w x h image; (seeds n x 2 f32,
    seeded bool) -- an entry that is not seeded keeps its own pixel."""
    px = np.ascontiguousarray(px, np.float32).reshape(-1, 2)
    R = np.ascontiguousarray(R, np.float64)
    if R.size != 9:
        raise ValueError("R must be 3 x 3")
    seeds = np.zeros_like(px)
    seeded = np.zeros(len(px), np.uint8)
    cs = camera.struct()
    check(_lib.load().rsvio_predict_seeds(C.byref(cs), ptr(R), ptr(px), len(px), w, h, ptr(seeds), ptr(seeded)))
    return seeds, seeded.astype(bool)


def detect_key_points(img: np.ndarray, grid_size: int, existing_xy: np.ndarray | None = None, cap: int = 4096):
    """New corners (k x 2 u32) and their FAST scores in the reference's cell scan order."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    ex = np.zeros((0, 2), np.float32) if existing_xy is None else np.ascontiguousarray(existing_xy, np.float32)
    out = np.zeros((cap, 2), np.uint32)
    score = np.zeros(cap, np.float32)
    n = C.c_int32(0)
    check(_lib.load().rsvio_detect_keypoints(ptr(img), w, h, grid_size, ptr(ex) if len(ex) else None, len(ex),
                                             ptr(out), ptr(score), cap, C.byref(n)))
    return out[:n.value].copy(), score[:n.value].copy()


FEATURE_DTYPE = np.dtype([("id", np.uint64), ("x", np.float32), ("y", np.float32), ("r", np.float32, 4)])

GATE_OFF, GATE_DROP_RIGHT, GATE_DROP_BOTH = 0, 1, 2


@dataclass
class StereoGate:
    """rsvio_stereo_gate: the epipolar gate of a tracker handle.  mode: GATE_DROP_RIGHT / GATE_DROP_BOTH
    (or "drop_right" / "drop_both"); max_error: the bound on e = |d_l . (E d_r)| of unit bearings;
    T_Cl_Cr: 4 x 4, the right camera's pose in the left camera's frame (x_l = R x_r + t)."""
    mode: int | str
    max_error: float
    T_Cl_Cr: np.ndarray

    def struct(self) -> _lib.StereoGate:
        g = _lib.StereoGate()
        g.mode = _lib.GATE_MODES[self.mode] if isinstance(self.mode, str) else int(self.mode)
        g.max_error = float(self.max_error)
        T = np.asarray(self.T_Cl_Cr, np.float64)
        if T.shape != (4, 4):
            raise ValueError("T_Cl_Cr must be 4 x 4")
        g.T_Cl_Cr[:] = T.reshape(16).tolist()
        return g


@dataclass
class GateCounts:
    n_pairs: int = 0      # ids in both cameras' maps before the gate
    n_rejected: int = 0   # of them, the ones the gate dropped
    n_invalid: int = 0    # of those, the ones without a bearing (a failed unprojection, RAY with s < 0)


@dataclass
class PredictionCounts:
    """rsvio_prediction_counts: per camera (left, right), the entries of the previous frame's lists
    whose search started at a predicted seed, and those that fell back to their own position."""
    n_seeded: tuple = (0, 0)
    n_unseeded: tuple = (0, 0)


def stereo_gate_lists(gate: StereoGate, convention_l, convention_r, ids_l, uv_l, ids_r, uv_r):
    """rsvio_stereo_gate_lists: the gate's device function on two lists with ascending ids (uv: the
    stored f32 unprojected coordinates); (keep_l, keep_r, err_r, GateCounts) with bool keeps and
    err_r NaN for an unpaired or invalid right entry."""
    from .camera import CONVENTIONS
    cl, cr = (CONVENTIONS[c] if isinstance(c, str) else int(c) for c in (convention_l, convention_r))
    ids_l, ids_r = np.ascontiguousarray(ids_l, np.uint64), np.ascontiguousarray(ids_r, np.uint64)
    uv_l = np.ascontiguousarray(uv_l, np.float32).reshape(-1, 2)
    uv_r = np.ascontiguousarray(uv_r, np.float32).reshape(-1, 2)
    if len(uv_l) != len(ids_l) or len(uv_r) != len(ids_r):
        raise ValueError("one coordinate pair per id")
    keep_l, keep_r = np.zeros(len(ids_l), np.uint8), np.zeros(len(ids_r), np.uint8)
    err_r = np.zeros(len(ids_r), np.float64)
    g, c = gate.struct(), _lib.GateCounts()
    check(_lib.load().rsvio_stereo_gate_lists(C.byref(g), cl, cr, ptr(ids_l), ptr(uv_l), len(ids_l), ptr(ids_r),
                                              ptr(uv_r), len(ids_r), ptr(keep_l), ptr(keep_r), ptr(err_r),
                                              C.byref(c)))
    return keep_l.astype(bool), keep_r.astype(bool), err_r, GateCounts(c.n_pairs, c.n_rejected, c.n_invalid)


class StereoPatchTracker:
    """Device-resident stereo patch tracker (one HIP stream per instance)."""

    def __init__(self, width: int, height: int, levels: int = 6, grid_size: int = 50,
                 optical_flow_max_iterations: int = 20, optical_flow_convergence_threshold: float = 0.01,
                 device: int = 0, max_features: int = 4096):
        lib = _lib.load()
        p = _lib.TrackerParams(width, height, levels, grid_size, optical_flow_max_iterations,
                               float(optical_flow_convergence_threshold), device, max_features)
        h = C.c_void_p()
        check(lib.rsvio_tracker_create(C.byref(p), C.byref(h)))
        self._h = h
        self.width, self.height, self.levels = width, height, levels
        self.cap = max_features
        self._out_l = np.zeros(max_features, FEATURE_DTYPE)
        self._out_r = np.zeros(max_features, FEATURE_DTYPE)
        self._n = (0, 0)

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().rsvio_tracker_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process_frame(self, left: np.ndarray, right: np.ndarray):
        """Returns (left_features, right_features) structured arrays sorted by id."""
        left = np.ascontiguousarray(left, np.uint8)
        right = np.ascontiguousarray(right, np.uint8)
        if left.shape != (self.height, self.width) or right.shape != left.shape:
            raise ValueError(f"expected {self.height}x{self.width} images")
        nl, nr = C.c_size_t(0), C.c_size_t(0)
        rc = _lib.load().rsvio_tracker_process_frame(self._h, ptr(left), ptr(right), self.width,
                                                     ptr(self._out_l), self.cap, C.byref(nl),
                                                     ptr(self._out_r), self.cap, C.byref(nr))
        self._n = (nl.value, nr.value)  # RSVIO_ERR_CAPACITY still leaves consistent (truncated) lists
        check(rc)
        return self._out_l[:nl.value].copy(), self._out_r[:nr.value].copy()

    def process_frame_device(self, d_left: int, d_right: int):
        nl, nr = C.c_size_t(0), C.c_size_t(0)
        rc = _lib.load().rsvio_tracker_process_frame_device(self._h, d_left, d_right, ptr(self._out_l), self.cap,
                                                            C.byref(nl), ptr(self._out_r), self.cap, C.byref(nr))
        self._n = (nl.value, nr.value)
        check(rc)
        return nl.value, nr.value

    def submit(self, left: np.ndarray, right: np.ndarray):
        """First half of process_frame (rsvio_tracker_submit): enqueue the frame and return at
        once; the images are borrowed until collect()."""
        left = np.ascontiguousarray(left, np.uint8)
        right = np.ascontiguousarray(right, np.uint8)
        if left.shape != (self.height, self.width) or right.shape != left.shape:
            raise ValueError(f"expected {self.height}x{self.width} images")
        check(_lib.load().rsvio_tracker_submit(self._h, ptr(left), ptr(right), self.width))
        self._borrowed = (left, right)

    def submit_device(self, d_left: int, d_right: int):
        """rsvio_tracker_submit_device: device images (tightly packed), enqueued; collect() later."""
        check(_lib.load().rsvio_tracker_submit_device(self._h, d_left, d_right))

    def collect_device(self):
        """Second half (rsvio_tracker_collect): wait for the submitted frame; (n_left, n_right),
        the lists in self._out_l / self._out_r."""
        nl, nr = C.c_size_t(0), C.c_size_t(0)
        rc = _lib.load().rsvio_tracker_collect(self._h, ptr(self._out_l), self.cap, C.byref(nl), ptr(self._out_r),
                                               self.cap, C.byref(nr))
        self._n = (nl.value, nr.value)
        self._borrowed = None
        check(rc)
        return nl.value, nr.value

    def collect(self):
        """collect_device() returning (left_features, right_features) like process_frame."""
        nl, nr = self.collect_device()
        return self._out_l[:nl].copy(), self._out_r[:nr].copy()

    def get_track_points(self):
        """[{id: (x, y)} for cam0, cam1] like feature_tracker.rs:188-200."""
        l, r = self._out_l[:self._n[0]], self._out_r[:self._n[1]]
        return [{int(f["id"]): (float(f["x"]), float(f["y"])) for f in l},
                {int(f["id"]): (float(f["x"]), float(f["y"])) for f in r}]

    def set_cameras(self, left, right):
        """Attach the frame's camera models (rsvio.camera.Camera); every process_frame then also
        computes Frame::add_{left,right}_feature's undistorted coordinates on device."""
        if left is None:
            check(_lib.load().rsvio_tracker_set_cameras(self._h, None, None))
            self._cams = False
            return
        self._cl, self._cr = left.struct(), right.struct()
        check(_lib.load().rsvio_tracker_set_cameras(self._h, C.byref(self._cl), C.byref(self._cr)))
        self._cams = True

    def undistorted(self):
        """(n_l x 2, n_r x 2) f32 undistorted coordinates of the last process_frame's features."""
        ul = np.zeros((self._n[0], 2), np.float32)
        ur = np.zeros((self._n[1], 2), np.float32)
        check(_lib.load().rsvio_tracker_undistorted(self._h, ptr(ul), self._n[0], ptr(ur), self._n[1]))
        return ul, ur

    def set_stereo_gate(self, gate: StereoGate | None):
        """rsvio_tracker_set_stereo_gate: from the next frame on, every pair (an id in both cameras'
        maps) whose epipolar error exceeds gate.max_error, or that has no bearing, leaves cam1's map
        (GATE_DROP_RIGHT) or both maps (GATE_DROP_BOTH) at the end of the frame, on the device.  Needs
        set_cameras; None turns it off."""
        if gate is None:
            check(_lib.load().rsvio_tracker_set_stereo_gate(self._h, None))
            return
        g = gate.struct()
        check(_lib.load().rsvio_tracker_set_stereo_gate(self._h, C.byref(g)))

    def gate_counts(self) -> GateCounts:
        """The last collected frame's gate counters alone (they came back with its lists: no device call)."""
        c, n = _lib.GateCounts(), C.c_size_t(0)
        check(_lib.load().rsvio_tracker_gate_report(self._h, C.byref(c), None, None, 0, C.byref(n)))
        return GateCounts(c.n_pairs, c.n_rejected, c.n_invalid)

    def gate_report(self):
        """rsvio_tracker_gate_report of the last collected frame: (GateCounts, the rejected ids
        ascending, their errors -- NaN for a pair without a bearing); zeros and empty with the gate off."""
        c = self.gate_counts()
        ids, err = np.zeros(c.n_rejected, np.uint64), np.zeros(c.n_rejected, np.float64)
        n = C.c_size_t(0)
        if c.n_rejected:
            check(_lib.load().rsvio_tracker_gate_report(self._h, None, ptr(ids), ptr(err), len(ids), C.byref(n)))
        return c, ids, err

    def set_prediction(self, R_l, R_r=None):
        """rsvio_tracker_set_prediction: the rotation hints R_cur_prev (3 x 3) of the left and right
        camera for exactly the next frame enqueued (process_frame, or submit); set_prediction(None)
        clears a pending one.  Needs set_cameras."""
        if R_l is None:
            check(_lib.load().rsvio_tracker_set_prediction(self._h, None))
            return
        p = _lib.TrackPrediction()
        for name, R in (("R_l", R_l), ("R_r", R_r)):
            R = np.asarray(R, np.float64)
            if R.shape != (3, 3):
                raise ValueError(f"{name} must be 3 x 3")
            getattr(p, name)[:] = R.reshape(9).tolist()
        check(_lib.load().rsvio_tracker_set_prediction(self._h, C.byref(p)))

    def prediction_report(self):
        """rsvio_tracker_prediction_report of the last collected frame: (PredictionCounts, seeds_l,
        seeds_r) -- the seeds (k x 2 f32) in the order of the previous frame's lists; zeros and empty
        when that frame had no prediction."""
        c = _lib.PredictionCounts()
        check(_lib.load().rsvio_tracker_prediction_report(self._h, C.byref(c), None, 0, None, 0))
        n = [c.n_seeded[k] + c.n_unseeded[k] for k in range(2)]
        sl, sr = np.zeros((n[0], 2), np.float32), np.zeros((n[1], 2), np.float32)
        if n[0] + n[1]:
            check(_lib.load().rsvio_tracker_prediction_report(self._h, None, ptr(sl), n[0], ptr(sr), n[1]))
        return PredictionCounts(tuple(c.n_seeded), tuple(c.n_unseeded)), sl, sr

    def prediction_counts(self) -> "PredictionCounts":
        """The counters of prediction_report() alone."""
        c = _lib.PredictionCounts()
        check(_lib.load().rsvio_tracker_prediction_report(self._h, C.byref(c), None, 0, None, 0))
        return PredictionCounts(tuple(c.n_seeded), tuple(c.n_unseeded))

    def remove_id(self, ids):
        """StereoPatchTracker::remove_id (feature_tracker.rs:201-206): the device lists are
        compacted in order, so the cached lists are filtered the same way."""
        ids = np.ascontiguousarray(ids, np.uint64)
        check(_lib.load().rsvio_tracker_remove_ids(self._h, ptr(ids), len(ids)))
        n = []
        for out, k in ((self._out_l, self._n[0]), (self._out_r, self._n[1])):
            keep = out[:k][~np.isin(out[:k]["id"], ids)]
            out[:len(keep)] = keep
            n.append(len(keep))
        self._n = tuple(n)

    def device_lists(self):
        """rsvio_tracker_device_lists: the last collected frame's lists in place on the device, as
        (d_left, n_left, d_right, n_right, d_uv_left, d_uv_right) -- device addresses of the AoS
        rsvio_feature lists (ids 32 bytes apart) and, with cameras attached, of the undistorted
        float pairs (None without).  Valid until this tracker's next-but-one frame."""
        dl, dr, ul, ur = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        nl, nr = C.c_size_t(0), C.c_size_t(0)
        check(_lib.load().rsvio_tracker_device_lists(self._h, C.byref(dl), C.byref(nl), C.byref(dr), C.byref(nr),
                                                     C.byref(ul), C.byref(ur)))
        return dl.value, nl.value, dr.value, nr.value, ul.value, ur.value


def _image(img, h, w, slot):
    """(pointer, stride, on_device, keep-alive) of one H x W u8 image: a numpy array whose rows are
    contiguous (any row stride >= W) or a contiguous torch uint8 device tensor."""
    if not isinstance(img, np.ndarray) and hasattr(img, "data_ptr"):
        if not (img.is_cuda and img.is_contiguous() and tuple(img.shape) == (h, w) and img.element_size() == 1):
            raise ValueError(f"slot {slot}: device images must be contiguous {h}x{w} uint8 tensors")
        return img.data_ptr(), 0, 1, img
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.shape != (h, w):
        raise ValueError(f"slot {slot}: expected a {h}x{w} uint8 image")
    if a.strides[1] != 1 or a.strides[0] < w:
        a = np.ascontiguousarray(a)
    return a.__array_interface__["data"][0], a.strides[0], 0, a


class TrackerBatch:
    """rsvio_tracker_batch: one stereo frame per StereoPatchTracker tracked by one call -- one upload,
    three launches whatever the number of trackers, one read-back and one host wait; every list is
    byte for byte the tracker's own process_frame result, and each tracker is left as that call
    leaves it (batch and single calls may alternate).  The trackers are borrowed (they must outlive
    the batch; equal parameters, one device, each in one slot only)."""

    def __init__(self, trackers):
        self.trackers = list(trackers)
        self.n = len(self.trackers)
        arr = (C.c_void_p * max(self.n, 1))(*[t._h.value for t in self.trackers])
        h = C.c_void_p()
        check(_lib.load().rsvio_tracker_batch_create(arr, self.n, C.byref(h)))
        self._h = h
        self.status = [0] * self.n   # per slot, of the last call: what process_frame would have returned
        self.device_ms = 0.0         # of the last call: its launches by HIP events

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().rsvio_tracker_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _frames(self, lefts, rights):
        """The ctypes frame table (lists into each tracker's cached arrays) and what it points into."""
        if len(lefts) != self.n or len(rights) != self.n:
            raise ValueError(f"{len(lefts)} + {len(rights)} images for a batch of {self.n}")
        tab = (_lib.StereoFrame * self.n)()
        keep = []
        for i, (t, left, right) in enumerate(zip(self.trackers, lefts, rights)):
            pl, sl, dl, kl = _image(left, t.height, t.width, i)
            pr, sr, dr, kr = _image(right, t.height, t.width, i)
            if dl != dr:
                raise ValueError(f"slot {i}: one image on the host, the other on the device")
            if not dl and sl != sr:   # one row stride per frame
                kr = np.ascontiguousarray(kr)
                kl = np.ascontiguousarray(kl)
                pl, pr, sl = kl.__array_interface__["data"][0], kr.__array_interface__["data"][0], t.width
            c = tab[i]
            c.left, c.right, c.stride, c.on_device = pl, pr, sl, dl
            c.out_l, c.cap_l, c.out_r, c.cap_r = ptr(t._out_l), t.cap, ptr(t._out_r), t.cap
            keep.append((kl, kr))
        return tab, keep

    def process_frames(self, lefts, rights):
        """[(left_features, right_features)] per slot, as each tracker's process_frame returns them.
        A slot's RSVIO_ERR_CAPACITY is reported in .status[i] (its lists are still consistent) and
        does not raise."""
        tab, keep = self._frames(lefts, rights)
        ms = C.c_double(0.0)
        rc = _lib.load().rsvio_tracker_batch_process_frames(self._h, C.addressof(tab), C.byref(ms))
        check(rc)
        del keep
        self.device_ms = ms.value
        self.status = [int(c.status) for c in tab]
        out = []
        for t, c in zip(self.trackers, tab):
            t._n = (int(c.n_l), int(c.n_r))
            out.append((t._out_l[:c.n_l].copy(), t._out_r[:c.n_r].copy()))
        return out
