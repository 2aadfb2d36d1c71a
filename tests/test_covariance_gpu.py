"""rsvio_ba_covariance on the device against two CPU references, both evaluated at the GPU's own
returned state (ba.state() substituted into the problem), so state differences do not enter:

* poses: numpy's inverse of the oracle's reduced camera system S at lambda = 0;
* poses and landmarks, independently of any Schur formula: the blocks of numpy's inverse of the
  whole Hessian, assembled from oracle.factor_linearize per observation (covariance_reference.py).

Metric: the scaled error max_ij |Sigma_gpu - Sigma_ref|_ij / sqrt(Sigma_ref,ii Sigma_ref,jj), per
matrix (the n x n pose matrix, each 3x3 landmark block; landmark variances reach 1e5).  Cap 1e-8:
the GPU's S differs from the oracle's by reassociation (a few eps; the parity test accepts
1e-9 max|S|), the inverse amplifies that by cond(S) <= 1.6e5 over these cases (staircase at 20
keyframes), so eps cond n ~ 1.1e-16 * 1.6e5 * 120 ~ 2e-9, taken with a 5x margin.  The two
references agree with each other to 1.2e-11 on the poses (tests/test_covariance_cpu.py).  Measured
on an MI355X: 2.6e-11 at most over all the tests below (the Huber case), 9.4e-12 over the sizes and
patterns.
"""
import functools

import numpy as np
import pytest

import covariance_reference as R

pytestmark = pytest.mark.gpu
CAP = 1e-8

SIZES = [(2, 30), (3, 40), (10, 200), (11, 200), (12, 200), (14, 200), (17, 300), (21, 400)]
PATTERNS = ["staircase", "two_ended", "full_span", "random_gaps", "two_fixed_mono"]


@functools.lru_cache(maxsize=None)
def _size_problem(n_kf, n_lm):
    from rsvio import synthetic as S
    return S.ba_problem(n_kf, n_lm, kf_per_lm=min(6, n_kf))


@functools.lru_cache(maxsize=None)
def _pattern_problem(name):
    from rsvio import synthetic as S
    return S.ba_pattern_problem(name, 20)


def _adjuster(prob):
    from rsvio.ba import BundleAdjuster
    ba = BundleAdjuster(max_keyframes=21, max_landmarks=max(prob.n_lm, 1), max_observations=max(prob.n_obs, 1))
    ba.set_problem_from(prob)
    return ba


def _check(oracle, prob, ba, cov=None, huber_delta=2.0, what=""):
    """cov (default: a fresh all-landmark, full call) against both references at ba.state()."""
    from rsvio import ba as B
    if cov is None:
        cov = ba.covariance(landmarks=True, full=True, huber_delta=huber_delta)
    assert cov.status == B.COV_OK, (what, cov.status, cov.n_singular)
    pose, pw = ba.state()
    q = R.at_state(prob, pose, pw)
    free = np.nonzero(np.asarray(prob.kf_fixed) == 0)[0]
    n = 6 * len(free)
    assert cov.n_free == len(free) and cov.full.shape == (n, n) and cov.pose.shape == (prob.n_kf, 6, 6)
    ref_s = R.schur_pose_cov(oracle, q, huber_delta)
    ref_h, ref_lm, observed = R.dense_cov(oracle, q, huber_delta)
    e_s, e_h = R.scaled_err(cov.full, ref_s), R.scaled_err(cov.full, ref_h)
    e_lm = max((R.scaled_err(cov.landmarks[l], ref_lm[l]) for l in np.nonzero(observed)[0]), default=0.0)
    print(f"{what}: pose vs inv(S) {e_s:.3g}, vs inv(H) {e_h:.3g}, landmarks vs inv(H) {e_lm:.3g} "
          f"(cond S {np.linalg.cond(np.linalg.inv(ref_s)):.3g}), device {cov.device_ms * 1e3:.1f} us")
    # exactly symmetric, positive diagonal; the per-keyframe blocks are the diagonal blocks, bit for bit
    assert np.array_equal(cov.full, cov.full.T) and (np.diag(cov.full) > 0).all()
    for k in range(prob.n_kf):
        f = np.searchsorted(free, k)
        if prob.kf_fixed[k]:
            assert not cov.pose[k].any()
        else:
            assert np.array_equal(cov.pose[k], cov.full[6 * f:6 * f + 6, 6 * f:6 * f + 6])
    assert np.array_equal(cov.flags == B.COV_LM_OK, observed)
    assert (cov.flags[~observed] == B.COV_LM_NOT_OBSERVED).all() and not cov.landmarks[~observed].any()
    _, _, co = oracle.ba_build_system(q, 0.0, huber_delta)
    assert abs(cov.cost - co) <= 1e-10 * abs(co)
    assert e_s <= CAP and e_h <= CAP and e_lm <= CAP, (what, e_s, e_h, e_lm)
    return cov


@pytest.mark.parametrize("n_kf,n_lm", SIZES)
def test_sizes(gpu, oracle, n_kf, n_lm):
    """1, 2, 9, 10 free keyframes (the panel solver, its last two), 11 (the block solver's first,
    padded to 13), 13 and 16 (exact fits) and 20 (the maximum)."""
    prob = _size_problem(n_kf, n_lm)
    ba = _adjuster(prob)
    assert ba.run().status > 0
    _check(oracle, prob, ba, what=f"sizes {n_kf}x{n_lm}")
    ba.close()


@pytest.mark.parametrize("name", PATTERNS)
def test_patterns_at_20_keyframes(gpu, oracle, name):
    from rsvio import ba as B
    prob = _pattern_problem(name)
    ba = _adjuster(prob)
    assert ba.run().status > 0
    cov = _check(oracle, prob, ba, what=f"pattern {name}")
    if name == "two_fixed_mono":
        assert int((np.asarray(prob.kf_fixed) != 0).sum()) == 2
        assert int((cov.flags == B.COV_LM_NOT_OBSERVED).sum()) == 1
    if name == "full_span":
        assert np.bincount(np.unique(np.stack([prob.obs_lm, prob.obs_kf]), axis=1)[0]).max() == 20
    ba.close()


@pytest.mark.parametrize("how", ["initial", 1, 2, 3, 4, "default", "async"])
def test_exits_and_buffers(gpu, oracle, how):
    """The state the call relinearises is the one state() returns at every exit: before any run,
    MAX_ITERATIONS at and between chunk boundaries, the converged end, and after run_async / wait."""
    from rsvio.ba import lm_cfg
    prob = _size_problem(10, 200)
    ba = _adjuster(prob)
    if how == "async":
        ba.run_async()
        assert ba.wait().status > 0
    elif how == "default":
        assert ba.run().status > 0
    elif how != "initial":
        res = ba.run(lm_cfg(max_iterations=how))
        assert res.iterations == how
    _check(oracle, prob, ba, what=f"exit {how}")
    ba.close()


def _huber_problem():
    """test_cheirality_and_skip's (3, 20) problem with 10 % of the observations displaced by 10
    sigma (sigma = 0.5 px in normalised coordinates), so their Huber weights are < 1."""
    from rsvio import synthetic as S
    prob = S.ba_problem(n_kf=3, n_lm=20, kf_per_lm=2, seed=5, init_seed=6)
    rng = np.random.default_rng(77)
    hit = rng.choice(prob.n_obs, prob.n_obs // 10, replace=False)
    prob.obs_uv = prob.obs_uv.copy()
    prob.obs_uv[hit] += (10.0 * 0.5 / S.FX_LEFT) * np.where(rng.random((len(hit), 2)) < 0.5, -1.0, 1.0)
    prob.obs_uv = prob.obs_uv.astype(np.float32).astype(np.float64)
    return prob, hit


def test_huber_weights(gpu, oracle):
    """Huber at a delta the displaced observations exceed (delta = 3 sigma): weights < 1 enter H."""
    from rsvio import synthetic as S
    from rsvio.ba import lm_cfg
    prob, hit = _huber_problem()
    delta = 3.0 * 0.5 / S.FX_LEFT
    ba = _adjuster(prob)
    assert ba.run(lm_cfg(huber_delta=delta)).status > 0
    pose, pw = ba.state()
    q = R.at_state(prob, pose, pw)
    sq = np.array([float(r @ r) for r, _ in (oracle.factor_linearize(q.p_W[q.obs_lm[o]], q.pose7[q.obs_kf[o]],
                                                                     q.T_C_B2[q.obs_cam[o]], q.obs_uv[o]) for o in hit)])
    assert (sq > delta * delta).sum() >= len(hit) // 2  # the weights are really < 1
    _check(oracle, prob, ba, huber_delta=delta, what="huber")
    ba.close()


def test_cheirality_gives_landmark_singular(gpu, oracle):
    """One landmark pushed behind the cameras (J = 0 on the cheirality branch): V = 0 with
    observations -> LANDMARK_SINGULAR, n_singular 1, the output arrays keep their sentinel fill."""
    import ctypes as C
    import dataclasses

    from rsvio import _lib
    from rsvio import ba as B
    prob, _ = _huber_problem()
    bad = dataclasses.replace(prob, p_W=prob.p_W.copy())
    bad.p_W[0] = -bad.p_W[0] * 5.0
    ba = _adjuster(bad)
    cov = ba.covariance(landmarks=True, full=True)
    assert cov.status == B.COV_LANDMARK_SINGULAR and cov.n_singular == 1
    assert cov.pose is None and cov.full is None and cov.landmarks is None
    n = 6 * 2
    cc, cp = np.full((n, n), -7.0), np.full((3, 36), -7.0)
    lm, fl = np.full((bad.n_lm, 9), -7.0), np.full(bad.n_lm, 9, np.uint8)
    info = _lib.CovInfo()
    _lib.check(_lib.load().rsvio_ba_covariance(ba._h, 2.0, _lib.ptr(cc), _lib.ptr(cp), None, bad.n_lm, _lib.ptr(lm),
                                               _lib.ptr(fl), C.byref(info)))
    assert info.status == B.COV_LANDMARK_SINGULAR and info.n_singular == 1 and info.n_free == 2
    assert (cc == -7.0).all() and (cp == -7.0).all() and (lm == -7.0).all() and (fl == 9).all()
    ba.close()


def test_singular_camera_system(gpu):
    """Input used: set_problem refuses nothing about kf_fixed all zero (it needs only one free
    keyframe), so the window is test_sizes' (3, 40) with no fixed keyframe: the gauge is free, a
    pivot of S is not positive -> CAMERA_SINGULAR, outputs untouched."""
    import ctypes as C
    import dataclasses

    from rsvio import _lib
    from rsvio import ba as B
    prob = _size_problem(3, 40)
    free = dataclasses.replace(prob, kf_fixed=np.zeros(3, np.uint8))
    ba = _adjuster(free)
    n = 18
    cc, cp = np.full((n, n), -7.0), np.full((3, 36), -7.0)
    lm, fl = np.full((free.n_lm, 9), -7.0), np.full(free.n_lm, 9, np.uint8)
    info = _lib.CovInfo()
    _lib.check(_lib.load().rsvio_ba_covariance(ba._h, 2.0, _lib.ptr(cc), _lib.ptr(cp), None, free.n_lm, _lib.ptr(lm),
                                               _lib.ptr(fl), C.byref(info)))
    assert info.status == B.COV_CAMERA_SINGULAR and info.n_singular == 0 and info.n_free == 3
    assert (cc == -7.0).all() and (cp == -7.0).all() and (lm == -7.0).all() and (fl == 9).all()
    ba.close()


def test_selection(gpu):
    from rsvio import ba as B
    from rsvio._lib import RsvioError
    prob = _size_problem(10, 200)
    ba = _adjuster(prob)
    assert ba.run().status > 0
    every = ba.covariance(landmarks=True, full=True)
    rng = np.random.default_rng(5)
    idx = rng.permutation(prob.n_lm)[:37]
    idx = np.concatenate([idx, idx[3:4]])  # one repeat
    rng.shuffle(idx)
    some = ba.covariance(landmarks=idx)
    assert some.status == B.COV_OK and some.full is None and some.landmarks.shape == (38, 3, 3)
    assert np.array_equal(some.landmarks, every.landmarks[idx]) and np.array_equal(some.flags, every.flags[idx])
    assert np.array_equal(some.pose, every.pose)
    none = ba.covariance()  # n_sel = 0 with NULL landmark outputs
    assert none.status == B.COV_OK and none.landmarks is None and np.array_equal(none.pose, every.pose)
    for wrong in ([0, prob.n_lm], [-1]):
        with pytest.raises(RsvioError) as e:
            ba.covariance(landmarks=wrong)
        assert e.value.code == -1  # RSVIO_ERR_INVALID_ARG
    ba.close()


def test_state_untouched_and_repeatable(gpu):
    prob = _size_problem(12, 200)
    ba = _adjuster(prob)
    before0 = ba.state()
    c0 = ba.covariance(landmarks=True, full=True)  # at the initial state
    after0 = ba.state()
    assert np.array_equal(before0[0], after0[0]) and np.array_equal(before0[1], after0[1])
    assert np.array_equal(before0[0], prob.pose7) and np.array_equal(before0[1], prob.p_W)
    r1 = ba.run()
    s1 = ba.state()
    c1 = ba.covariance(landmarks=True, full=True)
    c2 = ba.covariance(landmarks=True, full=True)
    s2 = ba.state()
    assert np.array_equal(s1[0], s2[0]) and np.array_equal(s1[1], s2[1])
    for a, b in ((c1.full, c2.full), (c1.pose, c2.pose), (c1.landmarks, c2.landmarks), (c1.flags, c2.flags)):
        assert np.array_equal(a, b)
    assert c1.cost == c2.cost and not np.array_equal(c0.full, c1.full)
    r2 = ba.run()  # after covariance calls: the solve of a fresh handle, bit for bit
    s3 = ba.state()
    fresh = _adjuster(prob)
    rf = fresh.run()
    sf = fresh.state()
    for r in (r1, r2):
        assert (r.status, r.iterations, r.final_cost, r.initial_cost) == \
            (rf.status, rf.iterations, rf.final_cost, rf.initial_cost)
    for s in (s1, s3):
        assert np.array_equal(s[0], sf[0]) and np.array_equal(s[1], sf[1])
    ba.close()
    fresh.close()


def test_refused_in_flight_and_sharded(gpu):
    from rsvio.ba import BundleAdjuster
    from rsvio._lib import RsvioError
    prob = _size_problem(3, 40)
    ba = _adjuster(prob)
    ba.run_async()
    with pytest.raises(RsvioError) as e:
        ba.covariance()
    assert "in flight" in str(e.value)
    assert ba.wait().status > 0
    assert ba.covariance().status == 1
    ba.close()
    sh = BundleAdjuster(max_keyframes=21, max_landmarks=prob.n_lm, max_observations=prob.n_obs)
    sh.attach_comm(1, 0, BundleAdjuster.rccl_unique_id())
    sh.set_problem_from(prob)
    assert sh.run().status > 0
    with pytest.raises(RsvioError) as e:
        sh.covariance()
    assert "sharded" in str(e.value)
    sh.close()


def test_after_a_batch(gpu, oracle):
    from rsvio import synthetic as S
    from rsvio.ba import BundleBatch
    probs = [S.ba_problem(5, 60, kf_per_lm=5), S.ba_problem(12, 150, kf_per_lm=6)]
    wins = [_adjuster(p) for p in probs]
    batch = BundleBatch(wins)
    res = batch.run()
    for i, (w, p, r) in enumerate(zip(wins, probs, res)):
        assert r.status > 0
        _check(oracle, p, w, what=f"batch window {i}")
    batch.close()
    for w in wins:
        w.close()


def _mirror_frames():
    """tests/test_ba_gpu.py::test_sliding_window_mirror's frames."""
    from rsvio import synthetic as S
    from rsvio.ba import Frame
    prob = S.ba_problem(n_kf=4, n_lm=50, kf_per_lm=4, seed=8, init_seed=9)
    frames = []
    for k in range(prob.n_kf):
        T_B_W = np.eye(4)
        T_B_W[:3, :3] = S.rot_from_quat(prob.true_pose7[k, 3:])
        T_B_W[:3, 3] = prob.true_pose7[k, :3]
        fr = Frame(frame_id=k, T_W_B=np.linalg.inv(T_B_W), T_B_Cl=S.T_B_CL, T_B_Cr=S.T_B_CR)
        for o in np.nonzero(prob.obs_kf == k)[0]:
            (fr.left_features if prob.obs_cam[o] == 0 else fr.right_features).append(
                (int(prob.obs_lm[o]), tuple(prob.obs_uv[o])))
        frames.append(fr)
    return frames


def test_sliding_window(gpu, oracle):
    from rsvio import synthetic as S
    from rsvio.ba import SlidingWindow
    on, off = SlidingWindow(4, covariance=True), SlidingWindow(4)
    assert off.pose_covariance is None and off.landmark_covariance is None
    for sw in (on, off):
        for fr in _mirror_frames():
            sw.add_frame(fr)
    pose7, fixed, p_init, lm, kf, cam, uv, tcb, ids = on.build_problem()
    assert on.optimize() and off.optimize()
    # covariance=False (the one-shot solve path, as before) keeps nothing; covariance=True gives
    # the same window bit for bit, and the covariance of the applied state (the solver's)
    assert off.pose_covariance is None and off.landmark_covariance is None
    assert np.array_equal(on.map_ids, off.map_ids) and np.array_equal(on.map_pw, off.map_pw)
    assert all(np.array_equal(a.T_W_B, b.T_W_B) for a, b in zip(on.keyframes, off.keyframes))
    pose, pw = on.solver.state()
    prob = S.BAProblem(pose7, fixed, p_init, lm, kf, cam, uv, tcb, pose7, p_init)
    q = R.at_state(prob, pose, pw)
    ref_s = R.schur_pose_cov(oracle, q)
    ref_h, ref_lm, observed = R.dense_cov(oracle, q)
    assert on.pose_covariance.shape == (4, 6, 6) and not on.pose_covariance[0].any()
    for f in range(3):
        for ref in (ref_s, ref_h):
            assert R.scaled_err(on.pose_covariance[f + 1], ref[6 * f:6 * f + 6, 6 * f:6 * f + 6]) <= CAP
    assert sorted(on.landmark_covariance) == sorted(ids.tolist()) and observed.all()
    for l, fid in enumerate(ids.tolist()):
        assert R.scaled_err(on.landmark_covariance[fid], ref_lm[l]) <= CAP
