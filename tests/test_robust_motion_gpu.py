"""Robust motion tracking on the GPU (rsvio_track_motion_robust / _robust_tracker: three launches,
pnp_robust.hpp) against tests/robust_motion_reference.py.

Collapse: one hypothesis (the prior) with an all-accepting threshold is rsvio_track_motion bit for
bit.  Parity: every integer of the contract (pairs, the whole hyp_count array, the winner, both
masks, the LM's status and iteration count) equals the reference's and T_W_B agrees to 1e-9, the
tolerance test_motion_gpu.py uses against the oracle.  Every compared reference first passes the
margin guard (no squared error of any hypothesis within 1e-9 relative of the threshold; a winner
that is unique or tied only with hypotheses of the same inlier set), so a different rounding cannot
flip a decision."""
import ctypes as C
import math

import numpy as np
import pytest

import robust_motion_reference as R

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9
ALL = dict(n_hyp=1, inlier_sq_error=1e300)


@pytest.fixture(scope="module")
def motion(gpu):
    from rsvio.motion import MotionTracker
    mt = MotionTracker()
    yield mt
    mt.close()


class Scene:
    """A MotionFrame-like input built point by point: every map point (stored as f32) is observed by
    both cameras at the true pose, with `noise` on the normalised coordinates."""

    def __init__(self, p_cam, noise=1e-4, seed=0, unmapped=3, step=(0.03, 0.017), collinear=None):
        from rsvio import synthetic as S
        rng = np.random.default_rng(seed)
        self.T_W_B_last_kf = np.eye(4)
        self.T_W_B_last_kf[:3, 3] = [0.5, -0.2, 0.1]
        a = step[1]
        T = self.T_W_B_last_kf.copy()
        T[:3, :3] = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
        T[:3, 3] += [step[0], 0.0, 0.0]
        self.T_W_B_true = T
        T_C_B = [np.linalg.inv(S.T_B_CL), np.linalg.inv(S.T_B_CR)]
        self.T_C_B2 = np.stack([t.reshape(16) for t in T_C_B])
        p_cam = np.asarray(p_cam, np.float64).reshape(-1, 3)
        T_W_C = T @ S.T_B_CL
        W = p_cam @ T_W_C[:3, :3].T + T_W_C[:3, 3]
        if collinear:  # three map points EXACTLY collinear as stored: multiples of 1/64, w0, w0 + d, w0 + 2 d
            i0, i1, i2 = collinear
            w0, d = np.round(W[i0] * 64) / 64, np.round((W[i1] - W[i0]) * 64) / 64
            W[i0], W[i1], W[i2] = w0, w0 + d, w0 + 2 * d
        self.map_pw = W.astype(np.float32)
        n = len(p_cam)
        self.map_ids = (100 + 3 * np.arange(n)).astype(np.uint64)
        T_B_W = np.linalg.inv(T)
        lists = []
        for c in range(2):
            Tc = T_C_B[c] @ T_B_W
            pc = self.map_pw.astype(np.float64) @ Tc[:3, :3].T + Tc[:3, 3]
            uv = pc[:, :2] / pc[:, 2:3] + rng.normal(0.0, noise, (n, 2)) if n else np.zeros((0, 2))
            ids = np.concatenate([self.map_ids, (10 ** 6 + 2 * np.arange(unmapped) + c).astype(np.uint64)])
            uv = np.concatenate([uv, rng.uniform(-0.5, 0.5, (unmapped, 2))])
            lists.append((ids, uv.astype(np.float32)))
        (self.ids_l, self.uv_l), (self.ids_r, self.uv_r) = lists


def _points(n, seed=1, z=(3.5, 8.0)):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(*z, n)], 1)


def _run(motion, oracle, m, samples=None, lm=None, **rc):
    """The device call and the reference on the same input; the guard, then the comparison."""
    from rsvio.motion import RansacConfig, pnp_cfg
    rcfg = RansacConfig(**rc)
    motion.set_map(m.map_ids, m.map_pw)
    r = motion.track_motion_robust(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2, rcfg,
                                   cfg=pnp_cfg(**lm) if lm else None, samples=samples, want_counts=True)
    ref = R.run_case(oracle, m, n_hyp=rcfg.n_hyp, min_inliers=rcfg.min_inliers, seed=rcfg.seed,
                     inlier_sq_error=rcfg.inlier_sq_error, min_depth=rcfg.min_depth, samples=samples,
                     cfg=oracle.lm_cfg(**lm) if lm else None)
    assert R.margin_ok(ref, rcfg.inlier_sq_error)
    assert R.winner_ok(ref), ref.tied
    _same(r, ref)
    return r, ref


def _same(r, ref):
    assert (r.n_pairs, r.n_valid_pairs, r.n_valid_hyp) == (ref.n_pairs, ref.n_valid_pairs, ref.n_valid_hyp)
    assert np.array_equal(r.hyp_count, ref.hyp_count)
    assert (r.best_hyp, r.best_count, r.ransac_status) == (ref.best_hyp, ref.best_count, ref.ransac_status)
    assert np.array_equal(r.mask_l, ref.mask_l) and np.array_equal(r.mask_r, ref.mask_r)
    assert r.n_inliers == ref.n_inliers
    mo = r.motion
    assert (mo.status, mo.iterations, mo.n_observations, int(mo.is_keyframe)) == \
        (ref.status, ref.iterations, ref.n_observations, ref.is_keyframe)
    assert np.abs(mo.T_W_B - ref.T_W_B).max() <= POSE_TOL
    for a, b in ((mo.initial_cost, ref.initial_cost), (mo.final_cost, ref.final_cost)):
        assert abs(a - b) <= 1e-9 * max(1.0, abs(b))
    assert abs(mo.translation_norm - ref.translation_norm) <= 1e-9
    assert abs(mo.rotation_norm - ref.rotation_norm) <= 1e-9
    assert 0.0 < r.device_ms < 100.0


def _bits(m):
    return (m.status, m.iterations, m.n_observations, m.is_keyframe, m.initial_cost, m.final_cost,
            m.translation_norm, m.rotation_norm, m.T_W_B.tobytes())


# ---------------------------------------------------------------- exact collapse

@pytest.mark.parametrize("seed", [1, 2, 7])
def test_one_hypothesis_accepting_everything_is_track_motion(motion, seed):
    from rsvio import synthetic as S
    from rsvio.motion import RansacConfig
    m = S.motion_frame(seed=seed, outlier_frac=0.05 if seed == 7 else 0.0)
    motion.set_map(m.map_ids, m.map_pw)
    p = motion.track_motion(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2)
    r = motion.track_motion_robust(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2, RansacConfig(**ALL))
    assert p.success and p.iterations > 1
    assert _bits(r.motion) == _bits(p)
    assert r.best_hyp == 0 and r.best_count == p.n_observations == r.n_inliers
    assert r.n_pairs >= 3 and r.ransac_status == 1
    assert np.array_equal(np.flatnonzero(r.mask_l), np.flatnonzero(np.isin(m.ids_l, m.map_ids)))


def test_collapse_on_a_tracked_frame(gpu, stereo_frames):
    from rsvio import synthetic as S
    from rsvio.camera import EUROC
    from rsvio.motion import MotionTracker, RansacConfig
    trk = gpu.StereoPatchTracker(752, 480, levels=3, grid_size=50)
    trk.set_cameras(*EUROC)
    mt = MotionTracker()
    try:
        trk.process_frame(*stereo_frames[0])
        fl, fr = trk.process_frame(*stereo_frames[1])
        ul, ur = trk.undistorted()
        T_last = np.eye(4)
        T_C_B2 = np.stack([np.linalg.inv(S.T_B_CL).reshape(16), np.linalg.inv(S.T_B_CR).reshape(16)])
        ids = fl["id"].astype(np.uint64)
        rays = np.concatenate([ul.astype(np.float64), np.ones((len(ul), 1))], 1) * 4.0
        p_W = (S.T_B_CL[:3, :3] @ rays.T).T + S.T_B_CL[:3, 3]
        keep = np.arange(len(ids)) % 3 != 0
        mt.set_map(ids[keep], p_W[keep].astype(np.float32))
        p = mt.track_motion_tracker(trk, T_last, T_C_B2)
        r = mt.track_motion_tracker_robust(trk, T_last, T_C_B2, RansacConfig(**ALL))
        assert p.n_observations > 100
        assert _bits(r.motion) == _bits(p)
        assert len(r.mask_l) == len(fl) and len(r.mask_r) == len(fr)
        assert np.array_equal(r.mask_l != 0, np.isin(ids, ids[keep]))
        # the host-array entry point on the lists read back: the same bits and masks
        h = mt.track_motion_robust(ids, ul, fr["id"], ur, T_last, T_C_B2, RansacConfig(n_hyp=64, seed=3),
                                   want_counts=True)
        d = mt.track_motion_tracker_robust(trk, T_last, T_C_B2, RansacConfig(n_hyp=64, seed=3), want_counts=True)
        assert _bits(h.motion) == _bits(d.motion) and np.array_equal(h.hyp_count, d.hyp_count)
        assert np.array_equal(h.mask_l, d.mask_l) and np.array_equal(h.mask_r, d.mask_r)
    finally:
        mt.close()
        trk.close()


# ---------------------------------------------------------------- parity with the reference

def _explicit(n_hyp, n_pairs, seed):
    rng = np.random.default_rng(seed)
    s = np.stack([rng.choice(n_pairs, 3, replace=False) for _ in range(n_hyp)]).astype(np.int32)
    s[0] = -7   # row 0 is ignored
    return s


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("n_hyp", [2, 8, 64, 1024])
@pytest.mark.parametrize("n_map,n_feat", [(64, 24), (400, 120)])
def test_parity_with_the_reference(motion, oracle, n_map, n_feat, n_hyp, explicit):
    from rsvio import synthetic as S
    m = S.motion_frame(n_map=n_map, n_feat=n_feat, seed=21, noise_px=0.3, map_noise=0.001, outlier_frac=0.1)
    samples = _explicit(n_hyp, n_feat, 5) if explicit else None
    r, ref = _run(motion, oracle, m, samples=samples, n_hyp=n_hyp, seed=11, inlier_sq_error=1e-4, min_inliers=5)
    assert r.n_pairs == n_feat
    if n_hyp >= 8:   # (two hypotheses: the prior and one triple reach no consensus at 4.6 px)
        assert r.ransac_status == 1 and r.motion.success


def test_corrupted_frame_gets_the_labelled_mask_and_the_inlier_only_pose(motion, oracle):
    """The frame of test_robust_motion_cpu.py: 30 % of the observations displaced."""
    import dataclasses
    m, uv_l, uv_r, lab_l, lab_r = R.corrupted_frame()
    m = dataclasses.replace(m, uv_l=uv_l, uv_r=uv_r)
    r, ref = _run(motion, oracle, m, n_hyp=R.CORRUPT_HYP, seed=R.CORRUPT_SEED, inlier_sq_error=R.CORRUPT_SQ,
                  lm=R.CORRUPT_LM)
    assert np.array_equal(r.mask_l, lab_l) and np.array_equal(r.mask_r, lab_r)
    fit = oracle.track_motion(m.ids_l[lab_l == 1], uv_l[lab_l == 1], m.ids_r[lab_r == 1], uv_r[lab_r == 1], m.map_ids,
                              m.map_pw, m.T_W_B_last_kf, m.T_C_B2, cfg=oracle.lm_cfg(**R.CORRUPT_LM))
    assert np.abs(r.motion.T_W_B - np.array(fit.T_W_B[:]).reshape(4, 4)).max() <= POSE_TOL
    assert np.abs(r.motion.T_W_B - m.T_W_B_true).max() < 1e-3


# ---------------------------------------------------------------- edges

@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_pair_counts_up_to_three(motion, oracle, k):
    """k ids of the right list keep their map point: TOO_FEW_PAIRS (only the prior) until 3."""
    m = Scene(_points(12))
    m.ids_r = m.ids_r.copy()
    m.ids_r[k:12] += np.uint64(7 * 10 ** 6)
    samples = np.array([[0, 0, 0], [0, 1, 2], [2, 1, 0], [0, 2, 1]], np.int32)
    r, ref = _run(motion, oracle, m, samples=samples, n_hyp=4, inlier_sq_error=1e-2, min_inliers=5)
    assert r.n_pairs == k and r.ransac_status == (2 if k < 3 else 1)
    assert r.n_valid_hyp == (1 if k < 3 else 4) and r.motion.success
    if k < 3:
        assert r.best_hyp == 0


def test_invalid_hypotheses(motion, oracle):
    """A repeated index, an index out of range (not an error), a collinear triple, a pair with
    parallel rays and a pair nearer than min_depth each invalidate their hypothesis only."""
    p = _points(14, seed=4, z=(4.0, 8.0))
    p[0], p[1], p[2] = [0.0, 0.0, 4.0], [0.5, 0.25, 4.5], [1.0, 0.5, 5.0]
    m = Scene(p, collinear=(0, 1, 2))
    a, b = (m.map_pw[k].astype(np.float64) - m.map_pw[0] for k in (1, 2))
    assert not np.cross(a, b).any() and a.any()
    T = m.T_C_B2.reshape(2, 4, 4)
    # pair 3: the same body ray from both cameras
    d_b = np.array([0.05, -0.02, 1.0])
    for c, uv in enumerate((m.uv_l, m.uv_r)):
        d = T[c, :3, :3] @ d_b
        uv[3] = (d[:2] / d[2]).astype(np.float32)
    # pair 4: a point 2.5 m deep, nearer than min_depth = 3
    q = np.linalg.inv(T[0])[:3, :3] @ np.array([0.1, 0.1, 2.5]) + np.linalg.inv(T[0])[:3, 3]
    for c, uv in enumerate((m.uv_l, m.uv_r)):
        pc = T[c, :3, :3] @ q + T[c, :3, 3]
        uv[4] = (pc[:2] / pc[2]).astype(np.float32)
    samples = np.array([[9, 9, 9], [5, 5, 6], [5, 6, 14], [5, -1, 6], [0, 1, 2], [3, 5, 6], [4, 5, 6], [5, 6, 7],
                        [2 ** 31 - 1, 5, 6]], np.int32)
    r, ref = _run(motion, oracle, m, samples=samples, n_hyp=9, inlier_sq_error=1e-4, min_depth=3.0, min_inliers=5)
    assert r.n_pairs == 14 and r.n_valid_pairs == 12
    assert list(r.hyp_count[1:7]) == [-1] * 6 and r.hyp_count[8] == -1 and r.hyp_count[7] > 5
    assert r.n_valid_hyp == 2


def test_observation_behind_the_camera_is_an_outlier(motion, oracle):
    """A map point behind both cameras whose coordinates are its projection through the centre: the
    squared error is ~0 at the true pose, the depth is negative."""
    p = _points(16, seed=6)
    p[5] = [0.3, -0.2, -4.0]
    m = Scene(p)
    r, ref = _run(motion, oracle, m, n_hyp=16, seed=2, inlier_sq_error=1e-4, min_inliers=5)
    assert r.mask_l[5] == 2 and r.mask_r[5] == 2
    assert r.n_inliers == 30 and r.motion.n_observations <= 30
    e2 = ref.sq_errors[-1]
    assert e2[5] < 1e-5   # only the depth test rejects it


def test_identical_sample_rows_tie_to_the_lower_h(motion, oracle):
    m = Scene(_points(20, seed=8))
    samples = np.array([[0, 0, 0], [18, 1, 2], [3, 9, 14], [3, 9, 14], [18, 1, 2]], np.int32)
    r, ref = _run(motion, oracle, m, samples=samples, n_hyp=5, inlier_sq_error=1e-4, min_inliers=5)
    assert r.hyp_count[1] == r.hyp_count[4] and r.hyp_count[2] == r.hyp_count[3]
    assert r.best_hyp in (1, 2) and r.best_hyp == min(ref.tied)


@pytest.mark.parametrize("n_l,n_r", [(32, 31), (32, 32), (33, 32), (2048, 2048)])
def test_joined_observation_counts(motion, oracle, n_l, n_r):
    """63, 64 and 65 joined observations (the ballot's tail) and 4,096, the capacity."""
    m = Scene(_points(n_l, seed=9), unmapped=0)
    m.ids_r, m.uv_r = m.ids_r[:n_r], m.uv_r[:n_r]
    r, ref = _run(motion, oracle, m, n_hyp=8, seed=4, inlier_sq_error=1e-4, min_inliers=5)
    assert r.n_pairs == n_r and int((r.mask_l != 0).sum() + (r.mask_r != 0).sum()) == n_l + n_r
    assert r.motion.success and r.n_inliers > 0.9 * (n_l + n_r)


def test_no_consensus(motion, oracle):
    """Every observation displaced and min_inliers = 10: the result of a frame without map points."""
    m = Scene(_points(24, seed=10))
    rng = np.random.default_rng(0)
    for uv in (m.uv_l, m.uv_r):
        uv += (rng.choice([-1.0, 1.0], uv.shape) * rng.uniform(0.5, 1.5, uv.shape)).astype(np.float32)
    r, ref = _run(motion, oracle, m, n_hyp=32, seed=1, inlier_sq_error=1e-4, min_inliers=10)
    assert r.ransac_status == -1 and r.motion.status == -2 and r.motion.is_keyframe
    assert np.array_equal(r.motion.T_W_B, np.eye(4)) and r.n_inliers == 0 and r.motion.n_observations == 0
    assert set(np.unique(r.mask_l[:24])) == {2}


def test_argument_errors(motion):
    from rsvio import RsvioError, _lib
    from rsvio import synthetic as S
    from rsvio.motion import RansacConfig, pnp_cfg
    m = S.motion_frame(n_map=64, n_feat=24, seed=5)
    motion.set_map(m.map_ids, m.map_pw)
    for bad in (dict(n_hyp=0), dict(n_hyp=1025), dict(n_hyp=-3), dict(inlier_sq_error=0.0),
                dict(inlier_sq_error=-1.0), dict(inlier_sq_error=float("nan"))):
        with pytest.raises(RsvioError) as e:
            motion.track_motion_robust(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2, RansacConfig(**bad))
        assert e.value.code == -1
    with pytest.raises(ValueError):
        motion.track_motion_robust(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2, RansacConfig(n_hyp=4),
                                   samples=np.zeros((3, 3), np.int32))
    # a NULL ransac cfg, and more than 4096 features
    Tl = np.ascontiguousarray(m.T_W_B_last_kf, np.float64)
    tcb = np.ascontiguousarray(m.T_C_B2, np.float64)
    cfg, res = pnp_cfg(), _lib.RobustMotionResult()
    lib = _lib.load()
    assert lib.rsvio_track_motion_robust(motion._h, None, None, 0, None, None, 0, Tl.ctypes.data, tcb.ctypes.data,
                                         C.byref(cfg), C.byref(motion.rule), None, None, None, None, None,
                                         C.byref(res)) == -1
    big = np.arange(5000, dtype=np.uint64)
    with pytest.raises(RsvioError) as e:
        motion.track_motion_robust(big, np.zeros((5000, 2)), big[:0], np.zeros((0, 2)), m.T_W_B_last_kf, m.T_C_B2)
    assert e.value.code == -4
    # an empty frame: no consensus, as track_motion's skipped frame
    r = motion.track_motion_robust(big[:0], np.zeros((0, 2)), big[:0], np.zeros((0, 2)), m.T_W_B_last_kf, m.T_C_B2)
    assert r.ransac_status == -1 and r.motion.status == -2 and r.motion.is_keyframe and r.n_pairs == 0


def test_two_calls_give_the_same_bits(motion):
    from rsvio import synthetic as S
    from rsvio.motion import RansacConfig
    m = S.motion_frame(n_map=400, n_feat=120, seed=13, outlier_frac=0.2)
    motion.set_map(m.map_ids, m.map_pw)
    rc = RansacConfig(n_hyp=256, seed=99)
    a, b = (motion.track_motion_robust(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2, rc,
                                       want_counts=True) for _ in range(2))
    assert _bits(a.motion) == _bits(b.motion) and a.motion.success
    assert np.array_equal(a.hyp_count, b.hyp_count) and a.best_hyp == b.best_hyp
    assert np.array_equal(a.mask_l, b.mask_l) and np.array_equal(a.mask_r, b.mask_r)
    assert (a.n_pairs, a.n_valid_pairs, a.n_valid_hyp, a.n_inliers) == (b.n_pairs, b.n_valid_pairs, b.n_valid_hyp,
                                                                         b.n_inliers)


# ---------------------------------------------------------------- Estimator

def _estimator(s, win, **kw):
    from rsvio.camera import Camera
    from rsvio.estimator import DeviceBackend, Estimator
    h, w = s.frames[0][0].shape
    cams = [Camera.opencv5(*p) for p in s.intrinsics]
    be = kw.pop("backend_cls", DeviceBackend)(w, h, cams, 6, 50, 20, 0.01, win, 0.05, 0.05, 0)
    return Estimator(w, h, cams, s.T_B_Cl, s.T_B_Cr, window=win, backend=be, **kw)


def test_estimator_collapse_reproduces_the_plain_estimator(gpu, scene_stream):
    from rsvio.motion import RansacConfig
    s, win = scene_stream
    runs = []
    for kw in ({}, dict(robust_motion=RansacConfig(**ALL))):
        est = _estimator(s, win, **kw)
        runs.append(list(est.run(s.frames)))
        est.close()
    assert len(runs[0]) == 24 and sum(r.pnp_status is not None for r in runs[0]) > 5
    for x, y in zip(*runs):
        assert (x.is_keyframe, x.pnp_status, x.pnp_iterations, x.pnp_cost, x.ba_status, x.ba_iterations) == \
               (y.is_keyframe, y.pnp_status, y.pnp_iterations, y.pnp_cost, y.ba_status, y.ba_iterations)
        assert np.array_equal(x.T_W_B, y.T_W_B)


def test_estimator_drop_outliers(gpu, scene_stream):
    """drop_outliers with pipelined is refused; otherwise the ids the robust call marks as outliers
    (here: a tenth of one frame's features, displaced by 0.1 before its motion tracking) have left
    the tracker when the next frame is tracked."""
    from rsvio.estimator import DeviceBackend, Estimator
    from rsvio.motion import RansacConfig
    s, win = scene_stream
    with pytest.raises(ValueError):
        Estimator(752, 480, None, s.T_B_Cl, s.T_B_Cr, backend=object(), pipelined=True,
                  robust_motion=RansacConfig(), drop_outliers=True)

    class Displacing(DeviceBackend):
        calls, displaced, feats, next_ids = 0, None, None, None

        def collect(self):
            self.feats = super().collect()
            if self.displaced is not None and self.next_ids is None:
                self.next_ids = np.concatenate([self.feats[0][0], self.feats[1][0]])
            return self.feats

        def track_motion_robust(self, T_last, T_C_B2, ransac):
            (ids_l, uv_l), (ids_r, uv_r) = self.feats
            uv_l = np.array(uv_l, np.float32)
            self.calls += 1
            if self.calls == 3:
                mapped = np.flatnonzero(np.isin(ids_l, self.map_ids))
                pick = mapped[::max(1, len(mapped) * 10 // len(ids_l))][:max(1, len(ids_l) // 10)]
                uv_l[pick] += np.float32(0.1)
                self.displaced = np.asarray(ids_l)[pick].astype(np.uint64)
            r = self.motion.track_motion_robust(ids_l, uv_l, ids_r, uv_r, T_last, T_C_B2, ransac)
            mo = r.motion
            return mo.status, mo.is_keyframe, mo.T_W_B, mo.iterations, mo.final_cost, r

        def set_map(self, ids, p_W):
            self.map_ids = np.asarray(ids, np.uint64)
            super().set_map(ids, p_W)

    est = _estimator(s, win, backend_cls=Displacing, robust_motion=RansacConfig(n_hyp=128), drop_outliers=True)
    dropped = None
    out = []
    for res in est.run(s.frames):
        out.append(res)
        if est.backend.calls == 3 and dropped is None:
            dropped = est.last_dropped.copy()
    be = est.backend
    assert len(out) == 24 and be.displaced is not None and len(be.displaced) >= 5
    assert set(be.displaced.tolist()) <= set(dropped.tolist())
    assert be.next_ids is not None and not np.isin(be.next_ids.astype(np.uint64), be.displaced).any()
    assert sum(r.pnp_status is not None and r.pnp_status > 0 for r in out) > 5
    est.close()
