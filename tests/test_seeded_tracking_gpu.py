"""Motion-predicted tracking on the GPU (rsvio_predict_seeds, rsvio_track_points_seeded,
rsvio_tracker_set_prediction / _prediction_report, Estimator(predict=...)) against
tests/seeded_tracking_reference.py, bit for bit.

Fixture: rsvio.synthetic.rotating_scene_pair at 376 x 240, L = 3, grid 30 (96 features of the left
camera), yaw 0.5 and 8 degrees; what the reference gives on it is pinned by
tests/test_seeded_tracking_cpu.py (at 8 degrees: unseeded 5, seeded 86, 88 seeds inside the image).
Every comparison is equality of bytes: the kernels restate the oracle's f32 / f64 operations in its
order, so there is no tolerance to choose."""
import numpy as np
import pytest

import seeded_tracking_reference as ref
from seeded_tracking_reference import GRID, H, LEVELS, W

pytestmark = pytest.mark.gpu

PARAMS = dict(levels=LEVELS, grid_size=GRID, optical_flow_max_iterations=20, optical_flow_convergence_threshold=0.01)
INVALID_ARG = -1


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _aff(feats):
    """A feature list's Affine2 states as the track maps hold them (n x 6 f32)."""
    a = np.zeros((len(feats), 6), np.float32)
    a[:, :4] = feats["r"]
    a[:, 4], a[:, 5] = feats["x"], feats["y"]
    return a


def _eucm_camera(oracle, convention=0):
    """An EUCM camera of the fixture's image size and focal length (TUM-VI's alpha / beta): with the
    reference, 88 of the fixture's 96 seeds stay inside the image at 8 degrees."""
    return oracle.camera(1, [230.0, 230.5, 187.0, 121.0, 0.6246, 1.0598], convention)


# ---------------------------------------------------------------- 1. seeds

@pytest.mark.parametrize("theta", [0.5, 8.0])
@pytest.mark.parametrize("kind", ["radtan_plane", "radtan_ray", "eucm"])
def test_predict_seeds_matches_reference(gpu, oracle, kind, theta):
    _, _, aff, cam, R, pair = ref.fixture(theta)
    if kind == "radtan_ray":
        cam = ref.opencv5_camera(pair.intrinsics[0], 1)
    elif kind == "eucm":
        cam = _eucm_camera(oracle)
    px = aff[:, 4:6]
    want, want_ok = ref.predict_seeds(cam, R, px, W, H)
    got, got_ok = gpu.predict_seeds(ref.rsvio_camera(cam), R, px, W, H)
    assert np.array_equal(got_ok, want_ok)
    assert _same(got, want)
    if theta == 8.0:   # some seeds leave the image and fall back to the own position
        assert 0 < int(want_ok.sum()) < len(px)
        assert _same(got[~got_ok], np.ascontiguousarray(px[~got_ok]))
    else:
        assert want_ok.all()


def test_predict_seeds_empty_and_invalid_pixels(gpu, oracle):
    _, _, _, cam, R, _ = ref.fixture(8.0)
    c = ref.rsvio_camera(cam)
    s, ok = gpu.predict_seeds(c, R, np.zeros((0, 2), np.float32), W, H)
    assert s.shape == (0, 2) and ok.shape == (0,)
    # pixels whose unprojection fails (EUCM outside its cone) or is NaN keep their own value, unseeded
    e = _eucm_camera(oracle)
    px = np.array([[1e4, 1e4], [np.nan, 5.0], [100.0, 100.0]], np.float32)
    want, want_ok = ref.predict_seeds(e, R, px, W, H)
    got, got_ok = gpu.predict_seeds(ref.rsvio_camera(e), R, px, W, H)
    assert np.array_equal(got_ok, want_ok) and list(want_ok) == [False, False, True]
    assert _same(got, want)


def test_predict_seeds_refuses_a_non_rotation(gpu):
    from rsvio import RsvioError
    _, _, aff, cam, R, _ = ref.fixture(8.0)
    c = ref.rsvio_camera(cam)
    for bad in (1.0001 * R, np.diag([1.0, -1.0, 1.0]) @ R, np.zeros((3, 3))):
        with pytest.raises(RsvioError) as e:
            gpu.predict_seeds(c, bad, aff[:, 4:6], W, H)
        assert e.value.code == INVALID_ARG


# ---------------------------------------------------------------- 2. the seeded kernel

@pytest.mark.parametrize("theta", [0.5, 8.0])
@pytest.mark.parametrize("n", [0, 1, 7, 96])
def test_seeded_kernel_matches_reference(gpu, theta, n):
    pyr0, pyr1, aff, cam, R, _ = ref.fixture(theta)
    seeds, _ = ref.predict_seeds(cam, R, aff[:, 4:6], W, H)
    aff, seeds = aff[:n], seeds[:n]
    want, want_ok = ref.track_points_seeded(pyr0, pyr1, W, H, LEVELS, aff, seeds)
    got, got_ok = gpu.track_points_seeded(pyr0, pyr1, W, H, LEVELS, aff, seeds)
    assert np.array_equal(got_ok, want_ok)
    assert _same(got, want)
    if n == 96:
        assert int(want_ok.sum()) >= 80 and not want_ok.all()


@pytest.mark.parametrize("levels,w,h,grid", [(1, W, H, GRID), (3, W, H, GRID), (6, 752, 480, 50)])
def test_seeded_kernel_levels(gpu, oracle, levels, w, h, grid):
    """Every instantiation family: one level, the fixture's three, six at 752 x 480 (both halves of the
    template build); and the collapse: every seed at its feature's position is rsvio_track_points."""
    pyr0, pyr1, aff, cam, R, _ = ref.fixture(8.0, 0, levels, w, h, grid)
    seeds, seeded = ref.predict_seeds(cam, R, aff[:, 4:6], w, h)
    want, want_ok = ref.track_points_seeded(pyr0, pyr1, w, h, levels, aff, seeds)
    got, got_ok = gpu.track_points_seeded(pyr0, pyr1, w, h, levels, aff, seeds)
    assert np.array_equal(got_ok, want_ok) and _same(got, want)
    assert want_ok.any() and not want_ok.all() and seeded.any() and not seeded.all()
    own = np.ascontiguousarray(aff[:, 4:6])
    plain, plain_ok = gpu.track_points(pyr0, pyr1, w, h, levels, aff)
    coll, coll_ok = gpu.track_points_seeded(pyr0, pyr1, w, h, levels, aff, own)
    assert np.array_equal(coll_ok, plain_ok) and _same(coll, plain)
    o, o_ok = oracle.track_points(pyr0, pyr1, w, h, levels, aff)
    assert np.array_equal(plain_ok, o_ok) and _same(plain, o)


@pytest.mark.parametrize("theta", [0.5])
@pytest.mark.parametrize("levels", [1, 3])
def test_collapse_at_a_small_yaw(gpu, theta, levels):
    """seeds = positions where the unseeded tracker keeps most tracks (both outcomes compared)."""
    pyr0, pyr1, aff, _, _, _ = ref.fixture(theta, 0, levels)
    plain, plain_ok = gpu.track_points(pyr0, pyr1, W, H, levels, aff)
    coll, coll_ok = gpu.track_points_seeded(pyr0, pyr1, W, H, levels, aff, np.ascontiguousarray(aff[:, 4:6]))
    assert np.array_equal(coll_ok, plain_ok) and _same(coll, plain)
    assert plain_ok.any() and not plain_ok.all()


def test_seeded_kernel_bad_seeds(gpu):
    """Finite seeds outside the image, non-finite seeds (= the own position) and seeds some pixels
    wrong: a forward pass that converges somewhere and a backward pass that does not come home."""
    pyr0, pyr1, aff, cam, R, _ = ref.fixture(8.0)
    seeds, _ = ref.predict_seeds(cam, R, aff[:, 4:6], W, H)
    seeds = seeds.copy()
    own = aff[:, 4:6]
    outside = [(-50.0, 10.0), (W + 30.0, H / 2), (1e9, 1e9), (10.0, -1e5), (W - 1.0, H - 1.0), (0.0, 0.0), (-3e38, 3e38)]
    seeds[:len(outside)] = outside
    nonfinite = slice(10, 16)
    seeds[10] = (np.nan, own[10, 1])
    seeds[11] = (own[11, 0], np.nan)
    seeds[12] = (np.inf, 4.0)
    seeds[13] = (5.0, -np.inf)
    seeds[14] = (np.nan, np.nan)
    seeds[15] = (np.inf, np.nan)
    wrong = slice(20, 96)
    offs = np.array([(3, 0), (-2.5, 2), (5, -4), (8, 0), (0, -9), (12, 6), (1, 1), (20, 0)], np.float32)
    seeds[wrong] += offs[np.arange(76) % len(offs)]
    want, want_ok = ref.track_points_seeded(pyr0, pyr1, W, H, LEVELS, aff, seeds)
    got, got_ok = gpu.track_points_seeded(pyr0, pyr1, W, H, LEVELS, aff, seeds)
    assert np.array_equal(got_ok, want_ok) and _same(got, want)
    # the non-finite seeds give the seed-at-position result
    at_own, at_own_ok = gpu.track_points_seeded(pyr0, pyr1, W, H, LEVELS, aff, np.ascontiguousarray(own))
    assert np.array_equal(got_ok[nonfinite], at_own_ok[nonfinite]) and _same(got[nonfinite], at_own[nonfinite])
    # the wrong seeds: the reference's forward pass converges on more than its backward test accepts
    fwd_ok = np.array([ref.track_one_seeded(pyr0, pyr1, W, H, LEVELS, a, s, 20, 0.01)[0]
                       for a, s in zip(aff[wrong], seeds[wrong])])
    assert int((fwd_ok & ~want_ok[wrong]).sum()) >= 10 and int(want_ok[wrong].sum()) >= 10
    assert not want_ok[:4].any()


# ---------------------------------------------------------------- 3. the tracker handle

def _cams(pair):
    from rsvio.camera import Camera
    return [Camera.opencv5(*p[:8]) for p in pair.intrinsics]


def _tracker(gpu, pair, cameras=True):
    t = gpu.StereoPatchTracker(W, H, **PARAMS)
    if cameras:
        t.set_cameras(*_cams(pair))
    return t


def _lists_equal(a, b):
    return _same(a[0], b[0]) and _same(a[1], b[1])


def _reference_frame(gpu, pair, prev, R, img_prev, img_cur, cam_index):
    """rsvio_build_pyramid, rsvio_predict_seeds and rsvio_track_points_seeded on one camera's previous
    list: (seeds, seeded, aff_out, valid)."""
    aff = _aff(prev)
    p0 = gpu.build_image_pyramid(img_prev, LEVELS)
    p1 = gpu.build_image_pyramid(img_cur, LEVELS)
    seeds, seeded = gpu.predict_seeds(_cams(pair)[cam_index], R, aff[:, 4:6], W, H)
    out, ok = gpu.track_points_seeded(p0, p1, W, H, LEVELS, aff, seeds)
    return seeds, seeded, out, ok


def _check_survivors(prev, new, out, ok):
    """Every id of the previous list is in the new list iff the reference says valid, with its affine."""
    pos = {int(i): k for k, i in enumerate(new["id"])}
    assert [int(i) in pos for i in prev["id"]] == list(ok)
    k = np.array([pos[int(i)] for i in prev["id"][ok]], np.int64)
    assert _same(_aff(new[k]), np.ascontiguousarray(out[ok]))


def test_handle_predicted_frame(gpu):
    pair = ref.scene_pair(8.0, W, H)
    R = pair.R_cur_prev
    (l0, r0), (l1, r1) = pair.frames
    A, B, Cn = _tracker(gpu, pair), _tracker(gpu, pair), _tracker(gpu, pair)
    a0, b0, c0 = A.process_frame(l0, r0), B.process_frame(l0, r0), Cn.process_frame(l0, r0)
    assert _lists_equal(a0, b0) and _lists_equal(a0, c0)
    assert A.prediction_counts().n_seeded == (0, 0)
    A.set_prediction(R, R)
    B.set_prediction(R, R)
    B.set_prediction(None)              # cleared: B launches what it always launched
    a1, b1, c1 = A.process_frame(l1, r1), B.process_frame(l1, r1), Cn.process_frame(l1, r1)
    assert _lists_equal(b1, c1)
    assert _same(B.undistorted()[0], Cn.undistorted()[0]) and _same(B.undistorted()[1], Cn.undistorted()[1])
    counts, sl, sr = A.prediction_report()
    kept = []
    for c, (prev, new, i0, i1, s) in enumerate(((a0[0], a1[0], l0, l1, sl), (a0[1], a1[1], r0, r1, sr))):
        seeds, seeded, out, ok = _reference_frame(gpu, pair, prev, R, i0, i1, c)
        _check_survivors(prev, new, out, ok)
        assert _same(s, seeds)
        assert counts.n_seeded[c] == int(seeded.sum()) and counts.n_unseeded[c] == int((~seeded).sum())
        assert 0 < counts.n_unseeded[c] < len(prev)
        kept.append(int(ok.sum()))
    # what the feature is for: the predicted handle keeps its tracks, the unpredicted one loses them
    lost = [int(np.isin(a0[c]["id"], c1[c]["id"]).sum()) for c in range(2)]
    # (the oracle tracker's 82 features per camera: 76 / 78 kept from the seeds, 5 / 7 without)
    assert min(kept) >= 70 and max(lost) <= 15
    assert B.prediction_counts().n_seeded == (0, 0) and B.prediction_counts().n_unseeded == (0, 0)
    for t in (A, B, Cn):
        t.close()


def test_handle_following_frame_is_unpredicted(gpu):
    pair = ref.scene_pair(8.0, W, H)   # (back by 8 degrees without a hint: a few tracks survive, most do not)
    R = pair.R_cur_prev
    (l0, r0), (l1, r1) = pair.frames
    A = _tracker(gpu, pair)
    A.process_frame(l0, r0)
    A.set_prediction(R, R)
    a1 = A.process_frame(l1, r1)
    assert sum(A.prediction_counts().n_seeded) > 0
    a2 = A.process_frame(l0, r0)        # the prediction was consumed by frame 1
    c, sl, sr = A.prediction_report()
    assert c.n_seeded == (0, 0) and c.n_unseeded == (0, 0) and len(sl) == 0 and len(sr) == 0
    for prev, new, i0, i1 in ((a1[0], a2[0], l1, l0), (a1[1], a2[1], r1, r0)):
        out, ok = gpu.track_points(gpu.build_image_pyramid(i0, LEVELS), gpu.build_image_pyramid(i1, LEVELS), W, H,
                                   LEVELS, _aff(prev))
        assert ok.any() and not ok.all()
        _check_survivors(prev, new, out, ok)
    A.close()


def test_handle_submit_collect_equals_process_frame(gpu):
    pair = ref.scene_pair(8.0, W, H)
    R = pair.R_cur_prev
    (l0, r0), (l1, r1) = pair.frames
    A, B = _tracker(gpu, pair), _tracker(gpu, pair)
    A.process_frame(l0, r0)
    B.submit(l0, r0)
    B.set_prediction(R, R)              # set while frame 0 is in flight: applies to the next submit
    B.collect()
    assert B.prediction_counts().n_seeded == (0, 0)
    A.set_prediction(R, R)
    a1 = A.process_frame(l1, r1)
    B.submit(l1, r1)
    b1 = B.collect()
    assert _lists_equal(a1, b1)
    ra, rb = A.prediction_report(), B.prediction_report()
    assert ra[0] == rb[0] and _same(ra[1], rb[1]) and _same(ra[2], rb[2]) and sum(ra[0].n_seeded) > 0
    # the report reads the collected frame's slot: a later submit does not disturb it
    B.submit(l0, r0)
    rb2 = B.prediction_report()
    assert rb2[0] == rb[0] and _same(rb2[1], rb[1]) and _same(rb2[2], rb[2])
    B.collect()
    assert B.prediction_counts().n_seeded == (0, 0)
    A.close()
    B.close()


def test_handle_refusals_and_first_frame(gpu):
    from rsvio import RsvioError, TrackerBatch
    pair = ref.scene_pair(8.0, W, H)
    R = pair.R_cur_prev
    (l0, r0), (l1, r1) = pair.frames
    bare = _tracker(gpu, pair, cameras=False)
    with pytest.raises(RsvioError) as e:
        bare.set_prediction(R, R)       # needs the cameras
    assert e.value.code == INVALID_ARG
    bare.close()
    A, D, ref_t = _tracker(gpu, pair), _tracker(gpu, pair), _tracker(gpu, pair)
    for bad in ((1.001 * R, R), (R, np.diag([1.0, 1.0, -1.0]))):
        with pytest.raises(RsvioError) as e:
            A.set_prediction(*bad)
        assert e.value.code == INVALID_ARG
    # a first-frame prediction is consumed without effect
    D.set_prediction(R, R)
    d0, t0 = D.process_frame(l0, r0), ref_t.process_frame(l0, r0)
    assert _lists_equal(d0, t0) and D.prediction_counts() == ref_t.prediction_counts()
    d1, t1 = D.process_frame(l1, r1), ref_t.process_frame(l1, r1)
    assert _lists_equal(d1, t1)
    # the batch refuses a handle with a pending prediction and leaves it pending
    A.process_frame(l0, r0)
    A.set_prediction(R, R)
    batch = TrackerBatch([A])
    with pytest.raises(RsvioError) as e:
        batch.process_frames([l1], [r1])
    assert e.value.code == INVALID_ARG
    a1 = A.process_frame(l1, r1)
    twin = _tracker(gpu, pair)
    twin.process_frame(l0, r0)
    twin.set_prediction(R, R)
    assert _lists_equal(a1, twin.process_frame(l1, r1)) and sum(A.prediction_counts().n_seeded) > 0
    # ... and, with nothing pending, runs as before and reports an unpredicted frame
    b2 = batch.process_frames([l0], [r0])[0]
    assert _lists_equal(b2, twin.process_frame(l0, r0))
    assert A.prediction_counts().n_seeded == (0, 0) and A.prediction_counts().n_unseeded == (0, 0)
    batch.close()
    for t in (A, D, ref_t, twin):
        t.close()


# ---------------------------------------------------------------- 4. the Estimator

THETA_EST = 4.0


@pytest.fixture(scope="module")
def yaw_stream():
    from rsvio import synthetic as S
    return S.rotating_scene_stream(4, THETA_EST, W, H)


def _estimator(stream, **kw):
    from rsvio.camera import Camera
    from rsvio.estimator import Estimator
    cams = [Camera.opencv5(*p) for p in stream.intrinsics]
    return Estimator(W, H, cams, stream.T_B_Cl, stream.T_B_Cr, levels=LEVELS, grid_size=GRID, window=3, **kw), cams


def _est_lists(est, r):
    t = est.backend.tracker
    return t._out_l[:r.n_left].copy(), t._out_r[:r.n_right].copy()


def test_estimator_external_prediction(gpu, yaw_stream):
    stream, d = yaw_stream
    est, cams = _estimator(stream, predict="external")
    twin = gpu.StereoPatchTracker(W, H, **PARAMS)
    twin.set_cameras(*cams)
    plain = gpu.StereoPatchTracker(W, H, **PARAMS)
    plain.set_cameras(*cams)
    # the convention, by the test's own formula: R_c = R_C_B delta_R_B R_B_C with delta_R_B = R_Bcur_Bprev
    Rc = [np.linalg.inv(T[:3, :3]) @ d @ T[:3, :3] for T in (stream.T_B_Cl, stream.T_B_Cr)]
    kept = [0, 0]
    for k, (left, right) in enumerate(stream.frames):
        r = est.process_frame(left, right, d if k else None)
        if k:
            twin.set_prediction(*Rc)
        want = twin.process_frame(left, right)
        assert _lists_equal(_est_lists(est, r), want), k
        assert r.n_seeded == twin.prediction_counts().n_seeded
        assert (sum(r.n_seeded) > 0) == (k > 0)
        p = plain.process_frame(left, right)
        if k == 1:
            kept = [int(np.isin(first[0]["id"], want[0]["id"]).sum()), int(np.isin(first[0]["id"], p[0]["id"]).sum())]
        if k == 0:
            first = want
    assert kept[0] > 2 * max(kept[1], 1)   # the hint has the right sign: the inverse would lose the tracks too
    # the look-ahead run takes triples and gives the same frames
    est2, _ = _estimator(stream, predict="external")
    est3, _ = _estimator(stream, predict="external")
    seq = [est3.process_frame(l, r, d if k else None) for k, (l, r) in enumerate(stream.frames)]
    frames = [(l, r, d) if k else (l, r) for k, (l, r) in enumerate(stream.frames)]
    for a, b in zip(est2.run(frames), seq):
        assert (a.n_left, a.n_right, a.n_seeded, a.is_keyframe) == (b.n_left, b.n_right, b.n_seeded, b.is_keyframe)
        assert np.array_equal(a.T_W_B, b.T_W_B)
    for o in (est, est2, est3, twin, plain):
        o.close()


def test_estimator_without_prediction_is_unchanged(gpu, yaw_stream):
    import dataclasses
    stream, d = yaw_stream
    a, _ = _estimator(stream, predict=None)
    b, _ = _estimator(stream)
    for left, right in stream.frames:
        ra, rb = a.process_frame(left, right), b.process_frame(left, right)
        for f in dataclasses.fields(ra):
            va, vb = getattr(ra, f.name), getattr(rb, f.name)
            assert np.array_equal(va, vb) if isinstance(va, np.ndarray) else va == vb, f.name
        assert ra.n_seeded is None
        assert _lists_equal(_est_lists(a, ra), _est_lists(b, rb))
    with pytest.raises(ValueError):
        a.process_frame(*stream.frames[0], d)     # a hint needs predict="external"
    a.close()
    b.close()


def test_estimator_constant_velocity_and_native_refusals(gpu, yaw_stream):
    from rsvio.estimator import NativeEstimator
    stream, _ = yaw_stream
    est, _ = _estimator(stream, predict="constant_velocity")
    with pytest.raises(ValueError):
        est.run(stream.frames)
    # no earlier PnP poses (the window is still filling): the frames are not predicted
    for left, right in stream.frames[:3]:
        assert est.process_frame(left, right).n_seeded == (0, 0)
    with pytest.raises(ValueError):
        NativeEstimator(est.backend, stream.T_B_Cl, stream.T_B_Cr, window=3, predict="external")
    with pytest.raises(ValueError):
        _estimator(stream, predict="gyro")
    est.close()
