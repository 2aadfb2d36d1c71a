"""Landmark triangulation / gate, the parts that need no device: the ABI structs, argument checks
that run before any device call, and SlidingWindow's use of a solver's triangulate /
check_landmarks (selection mask = the landmarks that are not in the map, culling, defaults)."""
import ctypes as C

import numpy as np
import pytest


def test_struct_sizes():
    from rsvio import _lib
    assert C.sizeof(_lib.LandmarkGate) == 32
    assert C.sizeof(_lib.LandmarkInfo) == 32
    assert np.dtype(_lib.LANDMARK_INFO_DTYPE).itemsize == 32


def test_invalid_arguments_rejected_without_device():
    from rsvio import _lib
    from rsvio.ba import landmark_gate
    lib = _lib.load()
    g = landmark_gate()
    info = np.zeros(1, _lib.LANDMARK_INFO_DTYPE)
    assert lib.rsvio_ba_triangulate(None, None, 0, C.byref(g), None, None, None) == -1
    assert b"null handle" in lib.rsvio_last_error()
    assert lib.rsvio_ba_check_landmarks(None, 0, C.byref(g), _lib.ptr(info), None) == -1
    # the gate is checked before the handle is touched: any non-null address stands in for one
    fake = C.create_string_buffer(64)
    assert lib.rsvio_ba_triangulate(fake, None, 0, None, None, None, None) == -1
    assert b"null gate" in lib.rsvio_last_error()
    assert lib.rsvio_ba_check_landmarks(fake, 0, None, _lib.ptr(info), None) == -1
    for mode in (-1, 2):
        bad = landmark_gate(mode=mode)
        assert lib.rsvio_ba_triangulate(fake, None, 0, C.byref(bad), None, None, None) == -1
        assert b"mode" in lib.rsvio_last_error()
        assert lib.rsvio_ba_check_landmarks(fake, 0, C.byref(bad), _lib.ptr(info), None) == -1
    bad = landmark_gate(min_depth=2.0, max_depth=1.0)
    assert lib.rsvio_ba_triangulate(fake, None, 0, C.byref(bad), None, None, None) == -1
    assert b"min_depth" in lib.rsvio_last_error()


def test_default_gate():
    from rsvio.ba import TRI_FIRST_STEREO, landmark_gate
    g = landmark_gate()
    assert (g.mode, g.min_depth, g.max_depth, g.max_sq_error) == (TRI_FIRST_STEREO, 0.1, 100.0, 0.0)


# ---------------------------------------------------------------------------------------------
def _frames(prob, feature_id):
    """Keyframes whose features are a BAProblem's observations (landmark l -> feature_id(l))."""
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


class _Stub:
    """A solver object that records how SlidingWindow drives it."""

    def __init__(self, flagged=()):
        self.calls, self.mask, self.flagged = [], None, set(flagged)
        self.n_lm = 0

    def _res(self):
        from rsvio import _lib
        r = _lib.BaResult()
        r.status, r.iterations = 1, 3
        return r

    def set_problem(self, pose7, fixed, p_W, *rest):
        self.calls.append("set_problem")
        self.pose7, self.p_W, self.n_lm = np.array(pose7), np.array(p_W), len(p_W)

    def triangulate(self, mask=None, gate=None, want=False):
        self.calls.append("triangulate" if want else "triangulate_enqueue")
        self.mask = np.array(mask)
        return (self.p_W, None, int(self.mask.sum()) - 1) if want else None

    def run(self, cfg=None):
        self.calls.append("run")
        return self._res()

    def run_async(self, cfg=None):
        self.calls.append("run_async")

    def wait(self):
        self.calls.append("wait")
        return self._res()

    def state(self):
        return self.pose7.copy(), self.p_W.copy()

    def check_landmarks(self, gate=None):
        from rsvio import _lib
        from rsvio.ba import LM_DEPTH, LM_OK
        self.calls.append("check_landmarks")
        info = np.zeros(self.n_lm, _lib.LANDMARK_INFO_DTYPE)
        info["flags"] = [LM_DEPTH if i in self.flagged else LM_OK for i in range(self.n_lm)]
        return info, self.n_lm - len(self.flagged)

    def solve(self, pose7, fixed, p_W, *rest):
        self.calls.append("solve")
        return np.array(pose7), np.array(p_W), self._res()


@pytest.fixture(scope="module")
def small():
    from rsvio import synthetic as S
    return S.ba_problem(n_kf=3, n_lm=12, kf_per_lm=2, seed=5, init_seed=6)


def _window(prob, solver, in_map, **kw):
    from rsvio.ba import SlidingWindow
    fid = lambda l: 1000 - 7 * l  # noqa: E731 - descending ids: the map's order differs from the window's
    sw = SlidingWindow(prob.n_kf, solver=solver, **kw)
    for f in _frames(prob, fid):
        sw.add_frame(f)
    sw.map_points = {fid(l): prob.true_p_W[l].astype(np.float32) for l in in_map}
    return sw, fid


def test_mask_is_exactly_the_landmarks_outside_the_map(small):
    in_map = [0, 3, 4, 9]
    for use_async in (False, True):
        st = _Stub()
        sw, fid = _window(small, st, in_map, landmark_init="triangulate")
        ids = sw.build_problem()[-1]
        if use_async:
            assert sw.optimize_async() is None
            assert st.calls == ["set_problem", "triangulate_enqueue", "run_async"]  # no waiting call in between
            assert sw.finish() is True
        else:
            assert sw.optimize() is True
            assert st.calls == ["set_problem", "triangulate", "run"]
        want = np.array([0 if int(i) in {fid(l) for l in in_map} else 1 for i in ids], np.uint8)
        assert st.mask.dtype == np.uint8 and np.array_equal(st.mask, want)
        assert sw.last_triangulation == (int(want.sum()), int(want.sum()) - 1)
    # an empty map selects everything
    st = _Stub()
    sw, _ = _window(small, st, [], landmark_init="triangulate")
    sw.optimize()
    assert st.mask.all() and len(st.mask) == small.n_lm


def test_cull_removes_flagged_ids_in_ascending_order(small):
    flagged = {1, 4, 5, 10}
    st = _Stub(flagged)
    sw, _ = _window(small, st, [0, 1], cull=True)
    ids = sw.build_problem()[-1]
    assert sw.optimize() is True
    assert "check_landmarks" in st.calls and "triangulate" not in st.calls   # cull alone keeps the ray start
    keep = sorted(int(i) for k, i in enumerate(ids) if k not in flagged)
    assert sw.map_ids.tolist() == keep and len(sw.map_pw) == len(keep)
    assert np.all(np.diff(sw.map_ids) > 0)
    # the asynchronous path culls in finish()
    st = _Stub(flagged)
    sw, _ = _window(small, st, [0, 1], cull=True, landmark_init="triangulate")
    assert sw.optimize_async() is None and sw.finish() is True
    assert sw.map_ids.tolist() == keep


def test_options_need_a_solver_with_the_methods(small):
    from rsvio.ba import SlidingWindow

    class SolveOnly:   # what the oracle-backed solver offers
        def solve(self, *a):
            raise AssertionError

    for kw in ({"landmark_init": "triangulate"}, {"cull": True}):
        with pytest.raises(ValueError):
            SlidingWindow(3, solver=SolveOnly(), **kw)
    with pytest.raises(ValueError):
        SlidingWindow(3, solver=_Stub(), landmark_init="depth2")
    SlidingWindow(3, solver=SolveOnly())   # the defaults ask for nothing


def test_default_mode_never_triangulates(small):
    st = _Stub()
    sw, _ = _window(small, st, [0, 3])
    assert (sw.landmark_init, sw.cull) == ("ray", False)
    assert sw.optimize() is True
    assert st.calls == ["solve"] and sw.last_triangulation is None
    st = _Stub()
    sw, _ = _window(small, st, [0, 3])
    assert sw.optimize_async() is None and sw.finish() is True
    assert st.calls == ["set_problem", "run_async", "wait"]
