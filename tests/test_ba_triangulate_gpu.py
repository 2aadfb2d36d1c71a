"""Device-side landmark triangulation and the depth / reprojection gate (rsvio_ba_triangulate,
rsvio_ba_check_landmarks) against a numpy restatement of the formula, and the solves that start
from the triangulated points against the oracle's solve from the numpy-triangulated points.

Formula (include/rsvio_gpu.h): per observation o (keyframe k, camera c, normalised (u, v))
[R | t] = T_C_B[c] T_B_W(k), c_o = -R^T t, d_o = R^T (u, v, 1)^T / |.|, M_o = I - d_o d_o^T; per
landmark p = (sum M_o)^-1 sum M_o c_o; depths (R p + t)_z, squared errors |(x/z, y/z) - (u, v)|^2.

Tolerances (derived, not tuned).  Points: the forward error of the 3x3 solve is about
cond(A) 2^-53 relative; _np_landmarks asserts cond(A) <= 1e5 and |p| <= 15 m here, i.e. <= 2e-10 m,
and the tests take 1e-8 m absolute (about 50 x: FMA contraction, summation order).  Depths:
relative 1e-10.  Squared errors: absolute 1e-12.  Flags and counts: exact -- so that rounding
cannot flip one, _np_landmarks asserts that every gated quantity of the inputs (depths, errors,
det A) is at least 1e-3 (relative) away from its bound.  Solves: the bounds test_ba_gpu.py uses
(status and iteration count equal, poses 1e-7, points 1e-6).
"""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P_TOL, Z_RTOL, E_TOL, MARGIN = 1e-8, 1e-10, 1e-12, 1e-3
OK, TOO_FEW, DEGENERATE, DEPTH, ERROR, NOT_SELECTED = 1, 2, 4, 8, 16, 32
ALL_VIEWS, FIRST_STEREO = 0, 1


# ------------------------------------------------------------------------------------------
# the numpy reference
# ------------------------------------------------------------------------------------------
def _gate(mode=FIRST_STEREO, lo=0.1, hi=100.0, err=0.0):
    from rsvio.ba import landmark_gate
    return landmark_gate(mode, lo, hi, err)


def _away(x, bound):
    assert abs(x - bound) >= MARGIN * abs(bound), (x, bound)


def _np_landmarks(prob, gate, tri=True, mask=None, pose7=None, p_W=None):
    """(p n_lm x 3, n_obs, flags, min_depth, max_depth, max_sq_error) of rsvio_ba_triangulate
    (tri; p = the initial points after the call) or rsvio_ba_check_landmarks on (pose7, p_W)."""
    from rsvio.ba import se3_matrix
    pose7 = prob.pose7 if pose7 is None else pose7
    p_W = np.array(prob.p_W if p_W is None else p_W, np.float64)
    TCB = [np.asarray(T, np.float64).reshape(4, 4) for T in prob.T_C_B2]
    TBW = [se3_matrix(p) for p in pose7]
    n_lm = prob.n_lm
    order = np.lexsort((prob.obs_cam, prob.obs_kf, prob.obs_lm))      # (landmark, keyframe, camera)
    by_lm = [[] for _ in range(n_lm)]
    for i in order:
        by_lm[prob.obs_lm[i]].append(i)
    out_p = p_W.copy()
    n_obs, flags = np.zeros(n_lm, np.int32), np.zeros(n_lm, np.int32)
    zmin, zmax, emax = np.zeros(n_lm), np.zeros(n_lm), np.zeros(n_lm)
    for l in range(n_lm):
        if tri and mask is not None and not mask[l]:
            flags[l] = NOT_SELECTED
            continue
        used = by_lm[l]
        if tri and gate.mode == FIRST_STEREO:
            used = []
            for a, b in zip(by_lm[l], by_lm[l][1:]):
                if prob.obs_kf[a] == prob.obs_kf[b]:
                    used = [a, b]
                    break
        n_obs[l] = len(used)
        Rt = []
        for i in used:
            T = TCB[prob.obs_cam[i]] @ TBW[prob.obs_kf[i]]
            Rt.append((T[:3, :3], T[:3, 3], prob.obs_uv[i]))
        if tri:
            if len(used) < 2:
                flags[l] = TOO_FEW
                continue
            A, r = np.zeros((3, 3)), np.zeros(3)
            for R, t, uv in Rt:
                d = R.T @ np.array([uv[0], uv[1], 1.0])
                d /= np.linalg.norm(d)
                M = np.eye(3) - np.outer(d, d)
                A += M
                r += M @ (-R.T @ t)
            det, bound = np.linalg.det(A), 1e-12 * len(used) ** 3
            _away(det, bound)
            if not det > bound:
                flags[l] = DEGENERATE
                continue
            assert np.linalg.cond(A) <= 1e5
            p = np.linalg.solve(A, r)
            assert np.linalg.norm(p) <= 15.0
        else:
            if not used:
                flags[l] = TOO_FEW
                continue
            p = p_W[l]
        z, e = [], []
        for R, t, uv in Rt:
            pc = R @ p + t
            z.append(pc[2])
            e.append((pc[0] / pc[2] - uv[0]) ** 2 + (pc[1] / pc[2] - uv[1]) ** 2)
        zmin[l], zmax[l], emax[l] = min(z), max(z), max(e)
        for v in z:
            _away(v, gate.min_depth)
            _away(v, gate.max_depth)
        f = 0
        if zmin[l] < gate.min_depth or zmax[l] > gate.max_depth:
            f |= DEPTH
        if gate.max_sq_error > 0:
            for v in e:
                _away(v, gate.max_sq_error)
            if emax[l] > gate.max_sq_error:
                f |= ERROR
        flags[l] = f or OK
        if tri and flags[l] == OK:
            out_p[l] = p
    return out_p, n_obs, flags, zmin, zmax, emax


def _assert_info(info, ref):
    _, n_obs, flags, zmin, zmax, emax = ref
    assert np.array_equal(info["n_obs"], n_obs)
    assert np.array_equal(info["flags"], flags), np.nonzero(info["flags"] != flags)
    assert np.all(np.abs(info["min_depth"] - zmin) <= Z_RTOL * np.abs(zmin))
    assert np.all(np.abs(info["max_depth"] - zmax) <= Z_RTOL * np.abs(zmax))
    assert np.all(np.abs(info["max_sq_error"] - emax) <= E_TOL)


def _assert_tri(got, ref):
    pw, info, n_acc = got
    assert np.abs(pw - ref[0]).max() <= P_TOL
    rejected = ref[2] != OK
    assert np.array_equal(pw[rejected], ref[0][rejected])        # the uploaded values, bit for bit
    _assert_info(info, ref)
    assert n_acc == int((ref[2] == OK).sum())


def _adjuster(prob):
    from rsvio.ba import BundleAdjuster
    ba = BundleAdjuster(max_keyframes=21, max_landmarks=max(prob.n_lm, 1), max_observations=max(prob.n_obs, 1))
    ba.set_problem_from(prob)
    return ba


def _ray_start(prob):
    """The depth-2.0 rule (sliding_window.rs:248-262, rsvio_window_problem): a landmark starts on
    the ray of its first observation in window order (keyframe, left then right)."""
    from rsvio.ba import se3_matrix
    T_B_C = [np.linalg.inv(np.asarray(T).reshape(4, 4)) for T in prob.T_C_B2]
    T_W_B = [np.linalg.inv(se3_matrix(p)) for p in prob.pose7]
    p = np.zeros((prob.n_lm, 3))
    seen = np.zeros(prob.n_lm, bool)
    for i in np.lexsort((prob.obs_cam, prob.obs_kf)):
        l = prob.obs_lm[i]
        if not seen[l]:
            seen[l] = True
            T = T_W_B[prob.obs_kf[i]] @ T_B_C[prob.obs_cam[i]]
            p[l] = T[:3, :3] @ np.array([prob.obs_uv[i, 0], prob.obs_uv[i, 1], 2.0]) + T[:3, 3]
    assert seen.all()
    return p


@pytest.fixture(scope="module")
def small(gpu):
    """4 keyframes, 130 landmarks over 3 keyframes each: 390 slots in 7 waves (21 landmarks per
    wave), the landmarks starting at different lanes; on the depth-2 ray."""
    from rsvio import synthetic as S
    p = S.ba_problem(n_kf=4, n_lm=130, kf_per_lm=3)
    return dataclasses.replace(p, p_W=_ray_start(p))


@pytest.fixture(scope="module")
def cfg3(gpu):
    """The config-3 shape (10 keyframes, 2,000 landmarks, 24,000 observations) on the depth-2 ray."""
    from rsvio import synthetic as S
    p = S.ba_problem(pose_noise=(0.005, 0.001))
    return dataclasses.replace(p, p_W=_ray_start(p))


@pytest.fixture(scope="module")
def refs(small, cfg3):
    """numpy's triangulation of both problems in both modes, all landmarks selected (computed once)."""
    return {(name, mode): _np_landmarks(p, _gate(mode))
            for name, p in (("small", small), ("cfg3", cfg3)) for mode in (ALL_VIEWS, FIRST_STEREO)}


@pytest.fixture(scope="module")
def solves(oracle, small, cfg3, refs):
    """The oracle's solves from the ray start and from numpy's triangulated starts."""
    out = {}
    for name, p in (("small", small), ("cfg3", cfg3)):
        out[name, "ray"] = oracle.ba_solve(p)
        for mode in (ALL_VIEWS, FIRST_STEREO):
            out[name, mode] = oracle.ba_solve(dataclasses.replace(p, p_W=refs[name, mode][0]))
    return out


# ------------------------------------------------------------------------------------------
# 1-4: the kernel against numpy
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [ALL_VIEWS, FIRST_STEREO])
def test_both_modes_match_numpy(small, refs, mode):
    ref = refs["small", mode]
    assert np.all(ref[2] == OK) and ref[3].min() > 1.5 and ref[4].max() < 10.5
    assert np.array_equal(ref[1], np.full(130, 6 if mode == ALL_VIEWS else 2))
    ba = _adjuster(small)
    got = ba.triangulate(gate=_gate(mode), want=True)
    _assert_tri(got, ref)
    assert np.abs(got[0] - small.p_W).max() > 0.1                # the ray start was replaced
    again = ba.triangulate(gate=_gate(mode), want=True)          # idempotent and deterministic
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()
    assert got[2] == again[2] == 130
    ba.close()


@pytest.mark.parametrize("mode", [ALL_VIEWS, FIRST_STEREO])
def test_mask_selects_landmarks(small, mode):
    mask = (np.random.default_rng(5).permutation(130) < 65).astype(np.uint8)
    ba = _adjuster(small)
    full_pw, full_info, _ = ba.triangulate(gate=_gate(mode), want=True)
    ba.set_problem_from(small)                                   # back to the uploaded points
    pw, info, n_acc = ba.triangulate(mask, _gate(mode), want=True)
    off = mask == 0
    assert np.array_equal(pw[off], small.p_W[off])
    assert np.all(info["flags"][off] == NOT_SELECTED) and np.all(info["n_obs"][off] == 0)
    assert pw[~off].tobytes() == full_pw[~off].tobytes()
    assert info[~off].tobytes() == full_info[~off].tobytes()
    assert n_acc == 65
    _assert_tri((pw, info, n_acc), _np_landmarks(small, _gate(mode), mask=mask))
    ba.set_problem_from(small)                                   # another mask on the same handle
    _assert_tri(ba.triangulate(1 - mask, _gate(mode), want=True), _np_landmarks(small, _gate(mode), mask=1 - mask))
    ba.close()


def _edge_problem():
    """3 keyframes, a pure-translation stereo rig (the cameras' axes are the body's, 0.11 m apart),
    8 ordinary landmarks seen everywhere and 7 edge cases (indices 8..14, see the test)."""
    from rsvio import synthetic as S
    from rsvio.ba import se3_matrix
    base = S.ba_problem(n_kf=3, n_lm=4, kf_per_lm=3, seed=31, init_seed=32)
    TCB = [np.eye(4), np.eye(4)]
    TCB[1][0, 3] = -0.11
    TBW = [se3_matrix(p) for p in base.true_pose7]
    rng = np.random.default_rng(33)
    pts = np.stack([rng.uniform(-1.5, 1.5, 15), rng.uniform(-1, 1, 15), rng.uniform(3, 7, 15)], 1)
    obs = []

    def see(l, k, c, shift=0.0, as_cam=None):
        T = TCB[c if as_cam is None else as_cam] @ TBW[k]
        pc = T[:3, :3] @ pts[l] + T[:3, 3]
        obs.append((l, k, c, pc[0] / pc[2] + shift, pc[1] / pc[2]))

    for l in range(8):
        for k in range(3):
            see(l, k, 0), see(l, k, 1)
    # 8: no observation.  9: one mono observation.
    see(9, 1, 0)
    # 10: the left camera only, in two keyframes
    see(10, 0, 0), see(10, 2, 0)
    # 11: its only stereo slot is its last slot
    see(11, 0, 0), see(11, 1, 1), see(11, 2, 0), see(11, 2, 1)
    # 12: left and right (u, v) swapped: the rays meet behind the cameras
    see(12, 1, 0, as_cam=1), see(12, 1, 1, as_cam=0)
    # 13: the same (u, v) in both cameras: parallel rays
    see(13, 0, 0), see(13, 0, 1, as_cam=0)
    # 14: (u, v) in the third keyframe shifted by 0.05
    for k in range(3):
        see(14, k, 0, shift=0.05 if k == 2 else 0.0), see(14, k, 1, shift=0.05 if k == 2 else 0.0)
    o = np.array(obs)
    rng.shuffle(o)                                               # any order is allowed
    p0 = pts + rng.normal(0.0, 0.3, pts.shape)
    return S.BAProblem(pose7=base.true_pose7.copy(), kf_fixed=base.kf_fixed.copy(), p_W=p0,
                       obs_lm=o[:, 0].astype(np.int32), obs_kf=o[:, 1].astype(np.int32),
                       obs_cam=o[:, 2].astype(np.uint8),
                       obs_uv=o[:, 3:5].astype(np.float32).astype(np.float64),
                       T_C_B2=np.stack([T.reshape(16) for T in TCB]), true_pose7=base.true_pose7, true_p_W=pts)


def test_edge_landmarks(gpu):
    prob = _edge_problem()
    ba = _adjuster(prob)
    got = {}
    for key, gate in (("all", _gate(ALL_VIEWS)), ("stereo", _gate(FIRST_STEREO)),
                      ("all_err", _gate(ALL_VIEWS, err=1e-4))):
        ba.set_problem_from(prob)
        got[key] = ba.triangulate(gate=gate, want=True)
        _assert_tri(got[key], _np_landmarks(prob, gate))
    f = {k: v[1]["flags"] for k, v in got.items()}
    n = {k: v[1]["n_obs"] for k, v in got.items()}
    assert np.all(f["all"][:8] == OK) and np.all(f["stereo"][:8] == OK) and np.all(f["all_err"][:8] == OK)
    assert (f["all"][8], n["all"][8]) == (TOO_FEW, 0) and (f["stereo"][8], n["stereo"][8]) == (TOO_FEW, 0)
    assert (f["all"][9], n["all"][9]) == (TOO_FEW, 1) and (f["stereo"][9], n["stereo"][9]) == (TOO_FEW, 0)
    assert (f["all"][10], n["all"][10]) == (OK, 2) and (f["stereo"][10], n["stereo"][10]) == (TOO_FEW, 0)
    assert (f["all"][11], n["all"][11]) == (OK, 4) and (f["stereo"][11], n["stereo"][11]) == (OK, 2)
    # mode 1 picked keyframe 2's pair: the point of exactly those two observations
    two = (prob.obs_lm == 11) & (prob.obs_kf == 2)
    only = dataclasses.replace(prob, obs_lm=prob.obs_lm[two], obs_kf=prob.obs_kf[two], obs_cam=prob.obs_cam[two],
                               obs_uv=prob.obs_uv[two])
    assert np.abs(got["stereo"][0][11] - _np_landmarks(only, _gate(ALL_VIEWS))[0][11]).max() <= P_TOL
    for k in ("all", "stereo"):
        assert f[k][12] == DEPTH and got[k][1]["max_depth"][12] < 0.0
        assert np.array_equal(got[k][0][12], prob.p_W[12])       # the initial value is kept
        assert f[k][13] == DEGENERATE and np.array_equal(got[k][0][13], prob.p_W[13])
    assert f["all"][14] == OK and f["all_err"][14] == ERROR and f["stereo"][14] == OK
    assert np.array_equal(got["all_err"][0][14], prob.p_W[14])
    assert got["all"][2] == 11 and got["stereo"][2] == 10 and got["all_err"][2] == 10
    ba.close()


@pytest.mark.parametrize("mode", [ALL_VIEWS, FIRST_STEREO])
def test_longest_landmark(gpu, mode):
    """21 keyframes, every landmark in all of them with both cameras: 21 lanes and 42 observations
    per landmark, three landmarks per wave."""
    from rsvio import synthetic as S
    prob = S.ba_problem(n_kf=21, n_lm=5, kf_per_lm=21, seed=41, init_seed=42)
    ba = _adjuster(prob)
    ref = _np_landmarks(prob, _gate(mode))
    assert np.array_equal(ref[1], np.full(5, 42 if mode == ALL_VIEWS else 2)) and np.all(ref[2] == OK)
    _assert_tri(ba.triangulate(gate=_gate(mode), want=True), ref)
    ba.close()


# ------------------------------------------------------------------------------------------
# 5-6: solves from the triangulated start
# ------------------------------------------------------------------------------------------
def _assert_solve(res, state, ref):
    po, pwo, ro = ref
    assert (res.status, res.iterations) == (ro.status, ro.iterations)
    assert res.status > 0
    assert np.abs(state[0] - po).max() < 1e-7 and np.abs(state[1] - pwo).max() < 1e-6


@pytest.mark.parametrize("mode", [ALL_VIEWS, FIRST_STEREO])
@pytest.mark.parametrize("name", ["small", "cfg3"])
def test_solve_from_triangulated_start(request, solves, name, mode):
    prob = request.getfixturevalue(name)
    # a condition on the inputs: triangulation does not cost the oracle iterations
    assert solves[name, mode][2].iterations <= solves[name, "ray"][2].iterations
    ba = _adjuster(prob)
    ba.triangulate(gate=_gate(mode))
    res = ba.run()
    _assert_solve(res, ba.state(), solves[name, mode])
    ba.close()


def test_solve_async_without_outputs(small, solves):
    ba = _adjuster(small)
    assert ba.triangulate(gate=_gate(ALL_VIEWS), want=False) is None
    ba.run_async()
    res = ba.wait()
    _assert_solve(res, ba.state(), solves["small", ALL_VIEWS])
    ba.close()


def test_alternating_windows_on_one_handle(small, cfg3, solves):
    """Two windows taking turns on one handle: a stale arena (the other window's points or layout)
    would show in the solve."""
    from rsvio.ba import BundleAdjuster
    ba = BundleAdjuster(max_keyframes=21, max_landmarks=cfg3.n_lm, max_observations=cfg3.n_obs)
    for name, prob in (("small", small), ("cfg3", cfg3), ("small", small), ("cfg3", cfg3)):
        ba.set_problem_from(prob)
        ba.triangulate(gate=_gate(FIRST_STEREO))
        res = ba.run()
        _assert_solve(res, ba.state(), solves[name, FIRST_STEREO])
    ba.close()


def test_batch_of_triangulated_windows(small, solves):
    from rsvio import synthetic as S
    from rsvio.ba import BundleBatch
    other = S.ba_problem(n_kf=5, n_lm=90, kf_per_lm=3, seed=51, init_seed=52)
    other = dataclasses.replace(other, p_W=_ray_start(other))
    probs = [small, other]
    wins = [_adjuster(p) for p in probs]
    for w in wins:
        w.triangulate(gate=_gate(ALL_VIEWS))
    batch = BundleBatch(wins)
    res = batch.run()
    for w, p, r in zip(wins, probs, res):
        pose, pw = w.state()
        one = _adjuster(p)
        one.triangulate(gate=_gate(ALL_VIEWS))
        r1 = one.run()
        p1, w1 = one.state()
        one.close()
        assert (r.status, r.iterations) == (r1.status, r1.iterations) and r.status > 0
        assert np.abs(pose - p1).max() <= 1e-10 and np.abs(pw - w1).max() <= 1e-10
    _assert_solve(res[0], wins[0].state(), solves["small", ALL_VIEWS])
    batch.close()
    for w in wins:
        w.close()


# ------------------------------------------------------------------------------------------
# 7: check_landmarks
# ------------------------------------------------------------------------------------------
def test_check_landmarks(small, refs):
    from rsvio._lib import RsvioError
    # landmark 7's left and right observations swapped: the rays of a stereo pair meet behind it
    bad = dataclasses.replace(small, obs_uv=small.obs_uv.copy())
    mine = np.nonzero(small.obs_lm == 7)[0]
    for a in mine:
        b = [i for i in mine if small.obs_kf[i] == small.obs_kf[a] and i != a][0]
        bad.obs_uv[a] = small.obs_uv[b]
    ba = _adjuster(bad)
    gate = _gate()
    # before any solve: the initial state, as uploaded and after a triangulation
    info, n_ok = ba.check_landmarks(gate)
    ref = _np_landmarks(bad, gate, tri=False)
    _assert_info(info, ref)
    assert n_ok == int((ref[2] == OK).sum()) and np.all(info["n_obs"] == 6)
    wide = _gate(FIRST_STEREO, lo=-1e3, hi=1e3)                   # lets the point behind the cameras through
    pw, tinfo, _ = ba.triangulate(gate=wide, want=True)
    assert tinfo["flags"][7] == OK and tinfo["max_depth"][7] < 0.0
    info, _ = ba.check_landmarks(gate)
    _assert_info(info, _np_landmarks(bad, gate, tri=False, p_W=pw))
    assert info["flags"][7] == DEPTH
    # refused while a solve is in flight
    ba.run_async()
    for call in (lambda: ba.check_landmarks(gate), lambda: ba.triangulate(gate=gate),
                 lambda: ba.triangulate(gate=gate, want=True)):
        with pytest.raises(RsvioError) as e:
            call()
        assert e.value.code == -1 and "in flight" in str(e.value)
    res = ba.wait()
    # after the solve: the state get_state returns (a point behind a camera has no Jacobian, so
    # landmark 7 stays where it was)
    pose, pws = ba.state()
    info, n_ok = ba.check_landmarks(gate)
    ref = _np_landmarks(bad, gate, tri=False, pose7=pose, p_W=pws)
    _assert_info(info, ref)
    assert info["flags"][7] == DEPTH and n_ok == int((ref[2] == OK).sum())
    assert res.iterations >= 1
    # a wrong landmark count is an argument error
    g = _gate()
    import ctypes as C
    from rsvio import _lib
    assert _lib.load().rsvio_ba_triangulate(ba._h, None, 129, C.byref(g), None, None, None) == -1
    ba.close()
    ba = _adjuster(small)                                        # no problem uploaded on a fresh handle
    from rsvio.ba import BundleAdjuster
    fresh = BundleAdjuster(max_keyframes=4, max_landmarks=8, max_observations=64)
    with pytest.raises(RsvioError):
        fresh.check_landmarks(gate)
    fresh.close()
    ba.close()


# ------------------------------------------------------------------------------------------
# 8-9: SlidingWindow and Estimator
# ------------------------------------------------------------------------------------------
def _frames(prob, feature_id):
    from rsvio.ba import Frame, se3_matrix
    T_B_C = [np.linalg.inv(np.asarray(T).reshape(4, 4)) for T in prob.T_C_B2]
    frames = []
    for k in range(prob.n_kf):
        feats = [[], []]
        for i in np.nonzero(prob.obs_kf == k)[0]:
            feats[prob.obs_cam[i]].append((feature_id(int(prob.obs_lm[i])), tuple(np.float32(prob.obs_uv[i]))))
        frames.append(Frame(frame_id=k + 1, T_W_B=np.linalg.inv(se3_matrix(prob.pose7[k])), T_B_Cl=T_B_C[0],
                            T_B_Cr=T_B_C[1], left_features=feats[0], right_features=feats[1]))
    return frames


def _window(prob, **kw):
    """A full window of the problem's keyframes; every third landmark is in the map already."""
    from rsvio.ba import BundleAdjuster, SlidingWindow

    class Spy(BundleAdjuster):
        def state(self, out=None):
            self.last_state = super().state(out)
            return self.last_state

    fid = lambda l: 5000 - 3 * l  # noqa: E731
    sw = SlidingWindow(prob.n_kf, solver=Spy(max_keyframes=prob.n_kf, max_landmarks=prob.n_lm,
                                             max_observations=prob.n_obs), **kw)
    for f in _frames(prob, fid):
        sw.add_frame(f)
    sw.map_points = {fid(l): prob.true_p_W[l].astype(np.float32) for l in range(0, prob.n_lm, 3)}
    return sw


@pytest.fixture(scope="module")
def window_case(oracle, small):
    """The window's own problem (the ray-rule SlidingWindow builds it on the host), numpy's
    triangulation of the landmarks outside the map and the oracle's solve from there."""
    from rsvio import synthetic as S
    sw = _window(small)
    pose7, fixed, p_init, lm, kf, cam, uv, tcb, ids = sw.build_problem()
    in_map = np.isin(ids, sw.map_ids)
    sw.solver.close()
    prob = S.BAProblem(pose7, fixed, p_init, lm, kf, cam, uv, tcb, pose7, p_init)
    mask = (~in_map).astype(np.uint8)
    ref = _np_landmarks(prob, _gate(), mask=mask)
    assert 0 < mask.sum() < len(mask) and np.all(ref[2][mask == 1] == OK)
    return prob, ids, mask, oracle.ba_solve(dataclasses.replace(prob, p_W=ref[0]))


@pytest.mark.parametrize("use_async", [False, True])
def test_sliding_window_triangulate(small, window_case, use_async):
    from rsvio.ba import se3_matrix
    prob, ids, mask, (po, pwo, ro) = window_case
    sw = _window(small, landmark_init="triangulate")
    if use_async:
        assert sw.optimize_async() is None and sw.finish() is True
    else:
        assert sw.optimize() is True
    assert sw.last_triangulation == (int(mask.sum()), int(mask.sum()))
    r = sw.last_result
    assert (r.status, r.iterations) == (ro.status, ro.iterations) and r.status > 0
    pose, pw = sw.solver.last_state
    assert np.abs(pose - po).max() < 1e-7 and np.abs(pw - pwo).max() < 1e-6
    srt = np.argsort(ids)
    assert np.array_equal(sw.map_ids, ids[srt]) and np.array_equal(sw.map_pw, pw[srt].astype(np.float32))
    for f, p7 in zip(sw.keyframes, pose):
        assert np.abs(f.T_W_B - np.linalg.inv(se3_matrix(p7))).max() < 1e-12
    sw.solver.close()


def test_sliding_window_cull(small, window_case):
    """cull drops exactly the landmarks numpy flags on the solved state: here those a tight depth
    gate rejects (depths span 1.6 .. 10 m; a bound of 4 m splits them)."""
    prob, ids, mask, _ = window_case
    gate = _gate(FIRST_STEREO, 0.1, 4.0)
    sw = _window(small, landmark_init="triangulate", gate=gate, cull=True)
    assert sw.optimize() is True
    pose, pw = sw.solver.last_state
    ref = _np_landmarks(prob, gate, tri=False, pose7=pose, p_W=pw)
    keep = ref[2] == OK
    assert 0 < keep.sum() < len(keep)
    assert np.array_equal(sw.map_ids, np.sort(ids[keep]))
    assert np.array_equal(sw.map_pw, pw[keep][np.argsort(ids[keep])].astype(np.float32))
    sw.solver.close()


def test_estimator_passthrough(gpu, scene_stream):
    from rsvio.camera import Camera
    from rsvio.estimator import Estimator
    s, win = scene_stream
    h, w = s.frames[0][0].shape
    cams = [Camera.opencv5(*p) for p in s.intrinsics]
    runs = []
    for kw in ({"landmark_init": "triangulate"}, {"landmark_init": "triangulate"}, {}):
        est = Estimator(w, h, cams, s.T_B_Cl, s.T_B_Cr, window=win, **kw)
        assert est.window.landmark_init == kw.get("landmark_init", "ray")
        poses, solves_seen = [], 0
        for left, right in s.frames:
            r = est.process_frame(left, right)
            poses.append(r.T_W_B)
            if r.ba_status is not None:
                solves_seen += 1
                assert r.ba_status > 0
                if kw:
                    sel, acc = est.window.last_triangulation
                    assert 0 <= acc <= sel and (acc > 0 or sel == 0)
        assert solves_seen > 3
        runs.append(np.array(poses + est.trajectory()))
        est.close()
    assert np.array_equal(runs[0], runs[1])
    # (recorded, not asserted: the triangulated run's trajectory differs from the ray run's and
    # nothing here pins which is better)
    print("estimator passthrough: max |T_W_B(triangulate) - T_W_B(ray)| over the stream",
          np.abs(runs[0] - runs[2]).max() if runs[0].shape == runs[2].shape else "different keyframe counts")
