"""The stereo gate without a device: the numpy reference against closed forms, the C ABI's struct
sizes and the refusals decided before any device call, and the splits the GPU tests rely on --
the CPU oracle tracker (levels 2, grid 16) gated by the reference on the test sequences.

Rig of the sequences: R = I, t = (1, 0, 0), pinhole {120, 120, 80, 60}, max_error = 1 / 120 (one
pixel).  A = stereo_sequence(5, 160, 120, seed=1); H3 rolls the rows of the right image's right
half down by 3."""
import ctypes as C

import numpy as np
import pytest

import stereo_gate_reference as G


def _rig(rng):
    """A rig with a rotated right camera: T_Cl_Cr with a 3-degree rotation about a random axis."""
    a = rng.standard_normal(3)
    a /= np.linalg.norm(a)
    th = np.radians(3.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, [0.11, 0.004, -0.002]
    return T


def _views(T, p_l):
    """Points in the left frame as unit bearings of both cameras (x_l = R x_r + t)."""
    p_r = (p_l - T[:3, 3]) @ T[:3, :3]       # R^T (x_l - t), row-wise
    return p_l / np.linalg.norm(p_l, axis=1, keepdims=True), p_r / np.linalg.norm(p_r, axis=1, keepdims=True)


# ------------------------------------------------------------------ the reference against closed forms

def test_projected_points_have_no_error():
    rng = np.random.default_rng(0)
    T = _rig(rng)
    p = np.stack([rng.uniform(-2, 2, 200), rng.uniform(-1.5, 1.5, 200), rng.uniform(2, 9, 200)], 1)
    dl, dr = _views(T, p)
    assert G.pair_error(G.essential(T), dl, dr).max() < 1e-12


def test_displacement_across_the_epipolar_line_is_the_closed_form():
    """d_r moved by delta along the unit normal n of its epipolar plane (n = E^T d_l / |E^T d_l|,
    taken perpendicular to d_r) and renormalised: e = |E^T d_l| sin(delta)."""
    rng = np.random.default_rng(1)
    T = _rig(rng)
    E = G.essential(T)
    p = np.stack([rng.uniform(-2, 2, 100), rng.uniform(-1.5, 1.5, 100), rng.uniform(2, 9, 100)], 1)
    dl, dr = _views(T, p)
    line = dl @ E                                     # E^T d_l: d_r lies in its null plane
    n = line / np.linalg.norm(line, axis=1, keepdims=True)
    for delta in (1e-4, 1e-3, 8e-3):
        moved = np.cos(delta) * dr + np.sin(delta) * n
        want = np.linalg.norm(line, axis=1) * np.sin(delta)
        assert np.abs(G.pair_error(E, dl, moved) - want).max() < 1e-12


def test_error_does_not_depend_on_the_baseline_length():
    rng = np.random.default_rng(2)
    T = _rig(rng)
    dl, _ = _views(T, rng.uniform(1, 5, (50, 3)))
    dr = rng.standard_normal((50, 3))
    dr /= np.linalg.norm(dr, axis=1, keepdims=True)
    e = G.pair_error(G.essential(T), dl, dr)
    assert e.max() > 0.01
    for s in (0.5, 3.0, 1024.0):                      # powers of two scale t / |t| exactly, 3.0 to an ulp
        T2 = T.copy()
        T2[:3, 3] *= s
        assert np.abs(G.pair_error(G.essential(T2), dl, dr) - e).max() < 1e-15


def test_essential_of_the_test_rig():
    assert np.array_equal(G.essential(G.RIG_T), np.array([[0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]]))


def test_bearings_and_the_invalid_rules():
    uv = np.array([[0.3, -0.2], [np.nan, 0.1], [0.1, np.nan], [0.8, 0.7], [0.6, 0.8]], np.float32)
    d, ok = G.bearings(uv, G.PLANE)
    assert ok.tolist() == [True, False, False, True, True]
    assert np.allclose(np.linalg.norm(d[ok], axis=1), 1.0, atol=1e-15) and np.isnan(d[~ok]).all()
    x, y = np.float64(uv[0, 0]), np.float64(uv[0, 1])
    assert np.array_equal(d[0], np.array([x, y, 1.0]) / np.sqrt((x * x + y * y) + 1.0))
    d, ok = G.bearings(uv, G.RAY)
    s3 = (1.0 - np.float64(uv[3, 0]) ** 2) - np.float64(uv[3, 1]) ** 2
    s4 = (1.0 - np.float64(uv[4, 0]) ** 2) - np.float64(uv[4, 1]) ** 2
    assert s3 < 0                                     # 0.8^2 + 0.7^2 > 1: no bearing
    assert ok.tolist() == [True, False, False, False, bool(s4 >= 0)]
    assert d[0, 2] == np.sqrt((1.0 - x * x) - y * y)


def test_gate_lists_join_and_modes():
    """Unpaired ids at both ends and in the middle of either side are never touched; an invalid pair
    is rejected with e = NaN; DROP_RIGHT keeps every left entry."""
    ids_l = np.array([1, 3, 4, 6, 8, 9], np.uint64)
    ids_r = np.array([0, 3, 5, 6, 8, 11], np.uint64)
    uv_l = np.array([[0, 0], [0.1, 0.05], [0, 0], [0.2, 0.1], [np.nan, 0.0], [0, 0]], np.float32)
    uv_r = np.array([[0, 0], [0.0, 0.05], [0, 0], [0.1, 0.2], [0.0, 0.0], [0, 0]], np.float32)
    for mode in (G.DROP_RIGHT, G.DROP_BOTH):
        g = G.gate_lists(G.RIG_T, G.ONE_PIXEL, mode, G.PLANE, G.PLANE, ids_l, uv_l, ids_r, uv_r)
        assert (g.n_pairs, g.n_rejected, g.n_invalid) == (3, 2, 1)
        assert g.keep_r.tolist() == [True, True, True, False, False, True]
        assert g.keep_l.tolist() == ([True] * 6 if mode == G.DROP_RIGHT else [True, True, True, False, False, True])
        assert g.rejected_ids.tolist() == [6, 8] and g.rejected_err[0] > G.ONE_PIXEL and np.isnan(g.rejected_err[1])
        assert np.isnan(g.err_r[[0, 2, 4, 5]]).all() and g.err_r[1] < 1e-9


# ------------------------------------------------------------------ the C ABI without a device

def test_struct_sizes():
    from rsvio import _lib
    assert C.sizeof(_lib.StereoGate) == 144
    assert C.sizeof(_lib.GateCounts) == 16
    assert _lib.StereoGate.T_Cl_Cr.offset == 16 and _lib.StereoGate.max_error.offset == 8


def _gate(mode=1, max_error=G.ONE_PIXEL, T=G.RIG_T):
    from rsvio.tracker import StereoGate
    return StereoGate(mode, max_error, np.asarray(T, np.float64)).struct()


def test_refusals_that_need_no_device():
    from rsvio import _lib
    lib = _lib.load()
    g = _gate()
    assert lib.rsvio_tracker_set_stereo_gate(None, C.byref(g)) == -1
    assert lib.rsvio_tracker_gate_report(None, None, None, None, 0, None) == -1
    ids = np.array([1, 2, 3], np.uint64)
    uv = np.zeros((3, 2), np.float32)
    kl, kr, er = np.zeros(3, np.uint8), np.zeros(3, np.uint8), np.zeros(3)
    p = _lib.ptr

    def call(gate, cl=0, cr=0, il=ids, ir=ids, keep_l=kl):
        return lib.rsvio_stereo_gate_lists(None if gate is None else C.byref(gate), cl, cr, p(il), p(uv), len(il),
                                           p(ir), p(uv), len(ir), p(keep_l), p(kr), p(er), None)

    def refused(word, *a, **kw):
        assert call(*a, **kw) == -1
        assert word in lib.rsvio_last_error().decode(), lib.rsvio_last_error().decode()

    assert call(None) == -1
    assert call(g, keep_l=None) == -1                                    # a NULL output with entries
    refused("mode", _gate(mode=0))
    refused("mode", _gate(mode=3))
    refused("max_error", _gate(max_error=0.0))
    refused("max_error", _gate(max_error=-1.0))
    refused("max_error", _gate(max_error=np.inf))
    refused("max_error", _gate(max_error=np.nan))
    T = G.RIG_T.copy()
    T[1, 2] = np.nan
    refused("finite", _gate(T=T))
    T = G.RIG_T.copy()
    T[:3, 3] = 0.0
    refused("zero", _gate(T=T))
    T = G.RIG_T.copy()
    T[0, 0] = 1.0 + 3e-6
    refused("orthonormal", _gate(T=T))
    T[0, 0] = 1.0 + 1e-7                                                 # within 1e-6: reaches the id checks
    refused("ascending", _gate(T=T), ir=np.array([1, 3, 2], np.uint64))
    refused("convention", g, cl=2)
    refused("convention", g, cr=-1)
    refused("ascending", g, il=np.array([1, 1, 3], np.uint64))           # a repeated id
    refused("ascending", g, ir=np.array([3, 2, 5], np.uint64))


def test_python_layer():
    import rsvio
    from rsvio.estimator import FrameResult, StereoGateConfig
    from rsvio.tracker import StereoGate
    g = StereoGate("drop_both", 0.01, np.eye(4)).struct()
    assert g.mode == 2 and g.max_error == 0.01 and list(g.T_Cl_Cr) == np.eye(4).reshape(16).tolist()
    with pytest.raises(ValueError):
        StereoGate(1, 0.01, np.eye(3)).struct()
    assert rsvio.StereoGate is StereoGate and callable(rsvio.stereo_gate_lists)
    assert FrameResult(1, True, np.eye(4), 0, 0, None, None).n_gate_rejected is None
    assert StereoGateConfig(1, 0.01).mode == 1


def test_estimator_refuses_a_backend_without_a_gate():
    from rsvio import synthetic as S
    from rsvio.estimator import Estimator, StereoGateConfig

    class Solverless:
        solver = None

    with pytest.raises(ValueError, match="set_stereo_gate"):
        Estimator(160, 120, None, S.T_B_CL, S.T_B_CR, backend=Solverless(), stereo_gate=StereoGateConfig(1, 0.01))


# ------------------------------------------------------------------ the inputs of the GPU tests, pinned

@pytest.fixture(scope="module")
def seq_a():
    from rsvio import synthetic as S
    return list(S.stereo_sequence(5, 160, 120, seed=1))


def _split(run):
    return [(g.n_rejected, g.n_pairs) for g, _, _ in run]


def _clear_of_threshold(run):
    assert min(g.margin for g, _, _ in run) > 1e-6      # no decision a 1-ulp difference could flip
    assert all(g.n_invalid == 0 for g, _, _ in run)


def test_clean_sequence_rejects_nothing(oracle, seq_a):
    run = G.gated_oracle_run(oracle, seq_a, G.PINHOLE)
    assert _split(run) == [(0, 39), (0, 39), (0, 39), (0, 42), (0, 50)]
    _clear_of_threshold(run)


@pytest.mark.parametrize("cam,convention", [(G.PINHOLE, G.PLANE), (G.RADTAN, G.PLANE), (G.RADTAN, G.RAY),
                                            (G.EUCM, G.PLANE)])
def test_h3_every_frame_rejects_some(oracle, seq_a, cam, convention):
    run = G.gated_oracle_run(oracle, [(l, G.h3(r)) for l, r in seq_a], cam, convention)
    assert _split(run) == [(16, 36), (16, 37), (16, 37), (15, 38), (16, 43)]
    assert all(0 < g.n_rejected < g.n_pairs for g, _, _ in run)
    _clear_of_threshold(run)


def test_h3_from_frame_2_turns_good_tracks_bad(oracle, seq_a):
    run = G.gated_oracle_run(oracle, [(l, G.h3(r) if k >= 2 else r) for k, (l, r) in enumerate(seq_a)], G.PINHOLE)
    assert _split(run) == [(0, 39), (0, 39), (18, 38), (14, 37), (16, 43)]
    g, il, ir = run[2]
    assert len(il) == 39 and len(ir) == 38            # one id is unpaired
    assert set(g.rejected_ids.tolist()) & set(run[1][1].tolist())   # tracks that were good in frame 1
    _clear_of_threshold(run)


def test_rolled_right_image_and_wrong_baseline_reject_all(oracle, seq_a):
    run = G.gated_oracle_run(oracle, [(l, G.roll2(r)) for l, r in seq_a], G.PINHOLE)
    assert _split(run) == [(39, 39), (37, 37), (38, 38), (38, 38), (38, 38)]
    _clear_of_threshold(run)
    run = G.gated_oracle_run(oracle, seq_a, G.PINHOLE, T=G.RIG_T_Y)
    assert all(g.n_rejected == g.n_pairs > 30 for g, _, _ in run)
    _clear_of_threshold(run)


def test_small_sequences_reject_some(oracle):
    from rsvio import synthetic as S
    for seed in (3, 4, 5):
        frames = [(l, G.h3(r)) for l, r in S.stereo_sequence(5, 96, 64, seed=seed)]
        run = G.gated_oracle_run(oracle, frames, (0, [120.0, 120.0, 48.0, 32.0, 0, 0, 0, 0, 0]), w=96, h=64)
        assert all(2 <= g.n_rejected <= 4 and 6 <= g.n_pairs <= 10 for g, _, _ in run), _split(run)
        _clear_of_threshold(run)


def test_drop_right_rule_on_the_oracle(oracle, seq_a):
    """The DROP_RIGHT twin rule as set logic: the left list is the never-gated tracker's, and an id
    rejected once never comes back to the right list."""
    frames = [(l, G.h3(r) if k >= 2 else r) for k, (l, r) in enumerate(seq_a)]
    trk = oracle.StereoTracker(160, 120, 2, 16, 20, 0.01)
    cam = oracle.camera(*G.PINHOLE)
    rule = G.DropRight(G.RIG_T, G.ONE_PIXEL)
    dt = np.dtype([("id", np.uint64)])
    n_rej = []
    for left, right in frames:
        fl, fr = trk.process_frame(left, right)
        (il, xl), (ir, xr) = G.features(fl), G.features(fr)
        tl, tr = np.zeros(len(il), dt), np.zeros(len(ir), dt)
        tl["id"], tr["id"] = il, ir
        before = set(rule.removed)
        el, er, g = rule.step(tl, oracle.unproject(cam, xl)[0], tr, oracle.unproject(cam, xr)[0])
        assert np.array_equal(el["id"], il) and not before & set(er["id"].tolist())
        assert not set(g.rejected_ids.tolist()) & set(er["id"].tolist())
        n_rej.append(g.n_rejected)
    assert n_rej[:2] == [0, 0] and n_rej[2] == 18 and all(n > 0 for n in n_rej[2:])
    assert len(rule.removed) == sum(n_rej)
