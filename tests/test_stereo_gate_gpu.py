"""The tracker's stereo gate on the GPU (rsvio_tracker_set_stereo_gate, rsvio_tracker_gate_report,
rsvio_stereo_gate_lists) against tests/stereo_gate_reference.py and ungated twin handles.

Shapes: 160 x 120, 2 levels, grid 16 (96 x 64 for the small sequences).  Rig: R = I, t = (1, 0, 0),
focal 120, max_error = 1 / 120 (one pixel).  A = stereo_sequence(5, 160, 120, seed=1); H3 rolls the
rows of the right image's right half down by 3.  What the CPU oracle gives for these sequences under
the reference gate is pinned by tests/test_stereo_gate_cpu.py (H3: 16/36, 16/37, 16/37, 15/38, 16/43
rejected; from frame 2 on: 0/39, 0/39, 18/38, 14/37, 16/43; the rolled right image: every pair);
each test here asserts the split it relies on again, on the reference side, and that no pair lies
within 1e-6 * max_error of the threshold, so a 1-ulp difference cannot flip a decision.

Error bound: e is a dozen f64 operations on terms of magnitude <= 1, so the device and numpy agree
within 1e-14 absolute (max_error is of order 1e-3 to 1e-2); keep flags, ids and counts are equal."""
import ctypes as C

import numpy as np
import pytest

import stereo_gate_reference as G

pytestmark = pytest.mark.gpu

W, H = 160, 120
PARAMS = dict(levels=2, grid_size=16, optical_flow_max_iterations=20, optical_flow_convergence_threshold=0.01)
ERR_TOL = 1e-14
CAPACITY = -4


def _cams():
    from rsvio.camera import Camera
    return {
        "pinhole": (Camera.opencv5(120, 120, 80, 60), G.PLANE),
        "radtan_plane": (Camera.opencv5(*G.RADTAN[1]), G.PLANE),
        "radtan_ray": (Camera.opencv5(*G.RADTAN[1], convention="ray"), G.RAY),
        "eucm": (Camera.eucm(*G.EUCM[1]), G.PLANE),
    }


def _tracker(gpu, cam=None, mode=None, max_error=G.ONE_PIXEL, T=G.RIG_T, w=W, h=H):
    """A tracker with `cam` on both sides and, with a mode, the gate set."""
    from rsvio.tracker import StereoGate
    t = gpu.StereoPatchTracker(w, h, **PARAMS)
    if cam is not None:
        t.set_cameras(cam, cam)
    if mode:
        t.set_stereo_gate(StereoGate(mode, max_error, T))
    return t


def _bytes_equal(a, b):
    return len(a) == len(b) and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _same_lists(got, want, what=""):
    assert _bytes_equal(got[0], want[0]) and _bytes_equal(got[1], want[1]), what


def _same_report(rep, g, what=""):
    """A handle's gate_report against a reference GateResult."""
    c, ids, err = rep
    assert (c.n_pairs, c.n_rejected, c.n_invalid) == (g.n_pairs, g.n_rejected, g.n_invalid), what
    assert np.array_equal(ids, g.rejected_ids), what
    assert np.array_equal(np.isnan(err), np.isnan(g.rejected_err)), what
    ok = ~np.isnan(err)
    assert not ok.any() or np.abs(err[ok] - g.rejected_err[ok]).max() <= ERR_TOL, what


def _ref(twin, l, r, mode, conv, max_error=G.ONE_PIXEL, T=G.RIG_T):
    """The reference gate on a twin's frame (its lists and its undistorted coordinates)."""
    ul, ur = twin.undistorted()
    g = G.gate_lists(T, max_error, mode, conv, conv, l["id"], ul, r["id"], ur)
    assert g.margin > 1e-6
    return g, ul, ur


@pytest.fixture(scope="module")
def seq():
    """The rendered sequences (never modified)."""
    from rsvio import synthetic as S
    A = list(S.stereo_sequence(5, W, H, seed=1))
    flat = np.full((H, W), 77, np.uint8)
    return dict(
        clean=A,
        h3=[(l, G.h3(r)) for l, r in A],
        h3_from2=[(l, G.h3(r) if k >= 2 else r) for k, (l, r) in enumerate(A)],
        roll2=[(l, G.roll2(r)) for l, r in A],
        flatmid=[(A[0][0], G.h3(A[0][1])), (flat, flat), (A[1][0], G.h3(A[1][1])), (A[2][0], G.h3(A[2][1])),
                 (A[3][0], G.h3(A[3][1]))],
    )


# ---------------------------------------------------------------- 1. the stateless entry against the reference

LENGTHS = [0, 1, 63, 64, 65, 1024, 1025, 3000]


def _random_lists(rng, n_l, n_r, conv_l, conv_r, nan_frac=0.03):
    """Two ascending-id lists sharing about two thirds of their ids, ids beyond 2^32 included;
    coordinates within the unit disc mostly, some NaN, some (for RAY) with s < 0."""
    m = max(n_l, n_r)
    universe = np.sort(rng.choice(4 * m + 16, size=int(1.5 * m) + 2, replace=False)).astype(np.uint64)
    universe[len(universe) // 2:] += np.uint64(1 << 33)
    ids_l = np.sort(rng.choice(universe, n_l, replace=False))
    ids_r = np.sort(rng.choice(universe, n_r, replace=False))
    out = []
    for n, conv in ((n_l, conv_l), (n_r, conv_r)):
        uv = rng.uniform(-0.6, 0.6, (n, 2)).astype(np.float32)
        if conv == G.RAY and n:
            k = rng.random(n) < 0.05
            uv[k] = rng.uniform(0.75, 0.95, (int(k.sum()), 2)).astype(np.float32)   # x^2 + y^2 > 1
        uv[rng.random(n) < nan_frac, rng.integers(0, 2)] = np.nan
        out.append(uv)
    return ids_l, out[0], ids_r, out[1]


def _rotated_rig():
    th = np.radians(4.0)
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.02), -np.sin(0.02)], [0, np.sin(0.02), np.cos(0.02)]])
    T[:3, 3] = [0.11, -0.003, 0.004]
    return T


def _check_lists(gpu, T, max_error, mode, conv_l, conv_r, lists, what):
    from rsvio.tracker import StereoGate
    g = G.gate_lists(T, max_error, mode, conv_l, conv_r, *lists)
    assert g.margin > 1e-6, what
    keep_l, keep_r, err_r, c = gpu.stereo_gate_lists(StereoGate(mode, max_error, T), conv_l, conv_r, *lists)
    assert np.array_equal(keep_l, g.keep_l) and np.array_equal(keep_r, g.keep_r), what
    assert (c.n_pairs, c.n_rejected, c.n_invalid) == (g.n_pairs, g.n_rejected, g.n_invalid), what
    assert np.array_equal(np.isnan(err_r), np.isnan(g.err_r)), what
    ok = ~np.isnan(err_r)
    assert not ok.any() or np.abs(err_r[ok] - g.err_r[ok]).max() <= ERR_TOL, what
    return g


@pytest.mark.parametrize("n_l", LENGTHS)
def test_gate_lists_against_the_reference(gpu, n_l):
    """Every length pair; the conventions mixed left / right and the rig rotated, alternating."""
    rng = np.random.default_rng(100 + n_l)
    Ts = [G.RIG_T, _rotated_rig()]
    seen_rejected = seen_kept = seen_invalid = 0
    for k, n_r in enumerate(LENGTHS):
        conv_l, conv_r = (k >> 0) & 1, (k >> 1) & 1
        mode = G.DROP_BOTH if k % 2 else G.DROP_RIGHT
        lists = _random_lists(rng, n_l, n_r, conv_l, conv_r)
        g = _check_lists(gpu, Ts[(k >> 2) & 1], 0.05, mode, conv_l, conv_r, lists, f"n_l {n_l} n_r {n_r}")
        seen_rejected += g.n_rejected - g.n_invalid
        seen_kept += g.n_pairs - g.n_rejected
        seen_invalid += g.n_invalid
    if n_l >= 63:   # the cases are not trivial
        assert seen_rejected > 10 and seen_kept > 10 and seen_invalid > 0


def test_gate_lists_edges(gpu):
    """Unpaired ids at both ends and in the middle of either side, NaN on either side, RAY with
    s < 0, and thresholds that reject every pair and none."""
    ids_l = np.array([1, 3, 4, 6, 8, 9, 12, 1 << 40], np.uint64)
    ids_r = np.array([0, 3, 5, 6, 8, 9, 12, (1 << 40) + 1], np.uint64)
    uv_l = np.array([[0, 0], [0.1, 0.05], [0, 0], [0.2, 0.1], [np.nan, 0], [0.1, 0.2], [0.8, 0.7], [0, 0]], np.float32)
    uv_r = np.array([[0, 0], [0.0, 0.05], [0, 0], [0.1, 0.2], [0, 0], [0.3, np.nan], [0.1, 0.1], [0, 0]], np.float32)
    lists = (ids_l, uv_l, ids_r, uv_r)
    g = _check_lists(gpu, G.RIG_T, G.ONE_PIXEL, G.DROP_BOTH, G.RAY, G.PLANE, lists, "mixed")
    assert (g.n_pairs, g.n_rejected, g.n_invalid) == (5, 4, 3)     # 3 kept; 6 over the bound; 8, 9, 12 invalid
    assert g.keep_l.tolist() == [True, True, True, False, False, False, False, True]
    g = _check_lists(gpu, G.RIG_T, G.ONE_PIXEL, G.DROP_RIGHT, G.PLANE, G.PLANE, lists, "plane")
    assert (g.n_pairs, g.n_rejected, g.n_invalid) == (5, 4, 2) and g.keep_l.all()
    rng = np.random.default_rng(7)
    lists = _random_lists(rng, 1500, 1400, G.PLANE, G.PLANE, nan_frac=0.0)
    g = _check_lists(gpu, G.RIG_T, 1e-9, G.DROP_BOTH, G.PLANE, G.PLANE, lists, "all rejected")
    assert g.n_rejected == g.n_pairs > 500 and g.n_invalid == 0
    g = _check_lists(gpu, G.RIG_T, 1.5, G.DROP_BOTH, G.PLANE, G.PLANE, lists, "none rejected")
    assert g.n_rejected == 0 and g.keep_l.all() and g.keep_r.all()


@pytest.mark.parametrize("n_l,n_r", [(65, 64), (1024, 1025), (1025, 1024), (3000, 2900), (700, 3000)])
def test_frame_end_gate_compacts_maps_longer_than_the_block(gpu, n_l, n_r):
    """The frame end's whole gate (flags, compaction of ids, affines and coordinates, report) through
    its diagnostic entry on maps no synthetic frame reaches: ceil(n / 1024) entries per thread."""
    from rsvio import _lib
    from rsvio.tracker import StereoGate
    lib, p = _lib.load(), _lib.ptr
    rng = np.random.default_rng(n_l + n_r)
    for mode, conv_l, conv_r in ((G.DROP_BOTH, G.PLANE, G.RAY), (G.DROP_RIGHT, G.RAY, G.PLANE)):
        ids_l, uv_l, ids_r, uv_r = _random_lists(rng, n_l, n_r, conv_l, conv_r)
        aff_l = rng.standard_normal((n_l, 6)).astype(np.float32)
        aff_r = rng.standard_normal((n_r, 6)).astype(np.float32)
        g = G.gate_lists(G.RIG_T, 0.05, mode, conv_l, conv_r, ids_l, uv_l, ids_r, uv_r)
        assert g.margin > 1e-6 and 10 < g.n_rejected < g.n_pairs and g.n_invalid > 0
        out = [a.copy() for a in (ids_l, uv_l, aff_l, ids_r, uv_r, aff_r)]
        ml, mr, c = C.c_size_t(n_l), C.c_size_t(n_r), _lib.GateCounts()
        rep_ids, rep_err = np.zeros(n_r, np.uint64), np.zeros(n_r)
        gs = StereoGate(mode, 0.05, G.RIG_T).struct()
        _lib.check(lib.rsvio_dbg_stereo_gate_frame(C.byref(gs), conv_l, conv_r, p(out[0]), p(out[1]), p(out[2]),
                                                   C.byref(ml), p(out[3]), p(out[4]), p(out[5]), C.byref(mr),
                                                   p(rep_ids), p(rep_err), C.byref(c)))
        assert (c.n_pairs, c.n_rejected, c.n_invalid) == (g.n_pairs, g.n_rejected, g.n_invalid)
        assert (ml.value, mr.value) == (int(g.keep_l.sum()), int(g.keep_r.sum()))
        for got, src, keep, m in ((out[0], ids_l, g.keep_l, ml.value), (out[1], uv_l, g.keep_l, ml.value),
                                  (out[2], aff_l, g.keep_l, ml.value), (out[3], ids_r, g.keep_r, mr.value),
                                  (out[4], uv_r, g.keep_r, mr.value), (out[5], aff_r, g.keep_r, mr.value)):
            assert _bytes_equal(got[:m], src[keep]), (mode, n_l, n_r)
        _same_report((c, rep_ids[:c.n_rejected], rep_err[:c.n_rejected]), g)


# ---------------------------------------------------------------- 2. DROP_BOTH against a twin with remove_ids

@pytest.mark.parametrize("rig", ["pinhole", "radtan_plane", "radtan_ray", "eucm"])
def test_drop_both_equals_a_twin_with_remove_ids(gpu, seq, rig):
    cam, conv = _cams()[rig]
    trk, twin = _tracker(gpu, cam, G.DROP_BOTH), _tracker(gpu, cam)
    split = []
    for k, (left, right) in enumerate(seq["h3"]):
        got = trk.process_frame(left, right)
        tl, tr = twin.process_frame(left, right)
        g, _, _ = _ref(twin, tl, tr, G.DROP_BOTH, conv)
        twin.remove_id(g.rejected_ids)
        want = G.drop_both_lists(tl, tr, g.rejected_ids)
        _same_lists(got, want, f"frame {k}")
        for a, b in zip(trk.undistorted(), twin.undistorted()):
            assert _bytes_equal(a, b), f"frame {k}"
        assert trk.device_lists()[1::2][:2] == (len(want[0]), len(want[1]))
        _same_report(trk.gate_report(), g, f"frame {k}")
        split.append((g.n_rejected, g.n_pairs))
    assert split == [(16, 36), (16, 37), (16, 37), (15, 38), (16, 43)]
    trk.close()
    twin.close()


# ---------------------------------------------------------------- 3. DROP_RIGHT against a never-gated twin

def test_drop_right_equals_a_never_gated_twin(gpu, seq):
    cam, conv = _cams()["pinhole"]
    trk, twin = _tracker(gpu, cam, G.DROP_RIGHT), _tracker(gpu, cam)
    rule = G.DropRight(G.RIG_T, G.ONE_PIXEL, conv, conv)
    n_rej = []
    for k, (left, right) in enumerate(seq["h3_from2"]):
        got = trk.process_frame(left, right)
        tl, tr = twin.process_frame(left, right)
        ul, ur = twin.undistorted()
        want_l, want_r, g = rule.step(tl, ul, tr, ur)
        assert g.margin > 1e-6
        _same_lists(got, (want_l, want_r), f"frame {k}")
        gl, gr = trk.undistorted()
        assert _bytes_equal(gl, ul) and _bytes_equal(gr, ur[np.isin(tr["id"], want_r["id"])]), f"frame {k}"
        _same_report(trk.gate_report(), g, f"frame {k}")
        n_rej.append(g.n_rejected)
    assert n_rej[:3] == [0, 0, 18] and all(n > 0 for n in n_rej[2:])
    assert len(got[0]) > len(got[1]) > 0           # the rejected ids live on as mono points
    trk.close()
    twin.close()


# ---------------------------------------------------------------- 4. none rejected

@pytest.mark.parametrize("mode", [G.DROP_RIGHT, G.DROP_BOTH])
def test_none_rejected_equals_the_ungated_handle(gpu, seq, mode):
    cam, conv = _cams()["pinhole"]
    trk, twin = _tracker(gpu, cam, mode), _tracker(gpu, cam)
    for k, (left, right) in enumerate(seq["clean"]):
        got, want = trk.process_frame(left, right), twin.process_frame(left, right)
        _same_lists(got, want, f"frame {k}")
        for a, b in zip(trk.undistorted(), twin.undistorted()):
            assert _bytes_equal(a, b)
        c, ids, err = trk.gate_report()
        n_pairs = len(np.intersect1d(want[0]["id"], want[1]["id"]))
        assert (c.n_pairs, c.n_rejected, c.n_invalid, len(ids), len(err)) == (n_pairs, 0, 0, 0, 0) and n_pairs >= 39
    trk.close()
    twin.close()


# ---------------------------------------------------------------- 5. all rejected under DROP_BOTH

def test_all_rejected_empties_the_maps_and_ids_go_on(gpu, seq):
    cam, _ = _cams()["pinhole"]
    trk = _tracker(gpu, cam, G.DROP_BOTH)
    assigned = 0
    for k, (left, right) in enumerate(seq["roll2"]):
        l, r = trk.process_frame(left, right)
        c, ids, err = trk.gate_report()
        assert c.n_pairs == c.n_rejected > 30 and c.n_invalid == 0 and len(l) == 0 and len(r) == 0
        assert ids.tolist() == list(range(assigned, assigned + c.n_pairs))   # new ids from the previous last_id
        assert (err > G.ONE_PIXEL).all()
        assigned += c.n_pairs
        assert trk.device_lists()[1::2][:2] == (0, 0) and trk.get_track_points() == [{}, {}]
    trk.close()


# ---------------------------------------------------------------- 6. look-ahead and device images

def _map_from(trk, fl):
    """A map for track_motion: the frame's left features at depth 2 in front of the left camera."""
    ul, _ = trk.undistorted()
    rays = np.concatenate([ul.astype(np.float64), np.ones((len(ul), 1))], 1) * 2.0
    return fl["id"].astype(np.uint64), rays.astype(np.float32)


T_C_B2 = np.stack([np.eye(4).reshape(16), np.linalg.inv(G.RIG_T).reshape(16)])   # body = left camera


def test_submit_collect_and_device_images_equal_process_frame(gpu, seq):
    import torch
    from rsvio.motion import MotionTracker
    from test_motion_edges_gpu import _bits
    cam, _ = _cams()["radtan_plane"]
    ref, look, dev = (_tracker(gpu, cam, G.DROP_BOTH) for _ in range(3))
    frames = seq["h3"]
    want = []
    for left, right in frames:
        l, r = ref.process_frame(left, right)
        want.append((l, r, ref.undistorted(), ref.gate_report()))
    assert all(0 < w[3][0].n_rejected < w[3][0].n_pairs for w in want)
    mt = MotionTracker()
    mt.set_map(*_map_from(ref, want[-1][0]))          # (ids persist: frame 4's left ids cover most of every frame)
    look.submit(*frames[0])
    for k in range(len(frames)):
        got = look.collect()
        if k + 1 < len(frames):
            look.submit(*frames[k + 1])               # the next frame is in flight from here on
        l, r, und, rep = want[k]
        _same_lists(got, (l, r), f"frame {k}")
        for a, b in zip(look.undistorted(), und):
            assert _bytes_equal(a, b), f"frame {k}"
        c, ids, err = look.gate_report()
        assert (c.n_pairs, c.n_rejected, c.n_invalid) == (rep[0].n_pairs, rep[0].n_rejected, rep[0].n_invalid)
        assert np.array_equal(ids, rep[1]) and _bytes_equal(err, rep[2]), f"frame {k}"
        assert look.device_lists()[1::2][:2] == (len(l), len(r))
        # the device lists of the collected frame, through their consumer
        one = mt.track_motion_tracker(look, np.eye(4), T_C_B2)
        host = mt.track_motion(l["id"], und[0], r["id"], und[1], np.eye(4), T_C_B2)
        assert _bits(one) == _bits(host) and one.n_observations > 10, f"frame {k}"
        dl, dr = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in frames[k])
        torch.cuda.synchronize()
        n = dev.process_frame_device(dl.data_ptr(), dr.data_ptr())
        assert n == (len(l), len(r)) and _bytes_equal(dev._out_l[:n[0]], l) and _bytes_equal(dev._out_r[:n[1]], r)
        assert dev.gate_counts() == look.gate_counts()
    for t in (ref, look, dev, mt):
        t.close()


# ---------------------------------------------------------------- 7. consumers of a gated frame

def test_remove_ids_and_motion_tracking_after_a_gated_frame(gpu, seq):
    from rsvio.motion import MotionTracker
    from test_motion_edges_gpu import _bits
    cam, conv = _cams()["pinhole"]
    trk, twin = _tracker(gpu, cam, G.DROP_BOTH), _tracker(gpu, cam)
    mt = MotionTracker()
    frames = seq["h3"]
    for k, (left, right) in enumerate(frames[:3]):
        l, r = trk.process_frame(left, right)
        tl, tr = twin.process_frame(left, right)
        g, _, _ = _ref(twin, tl, tr, G.DROP_BOTH, conv)
        assert 0 < g.n_rejected < g.n_pairs
        ul, ur = trk.undistorted()
        if k == 0:
            mt.set_map(*_map_from(trk, l))
        one = mt.track_motion_tracker(trk, np.eye(4), T_C_B2)
        host = mt.track_motion(l["id"], ul, r["id"], ur, np.eye(4), T_C_B2)
        assert _bits(one) == _bits(host) and one.n_observations > 10, f"frame {k}"
        # ids leave after the gated frame: the twin loses the rejected ones and the same extra ids
        extra = l["id"][1::8]
        assert 0 < len(extra) < len(l)
        trk.remove_id(extra)
        twin.remove_id(np.concatenate([g.rejected_ids, extra]))
        assert trk.get_track_points() == twin.get_track_points()
        for a, b in zip(trk.undistorted(), twin.undistorted()):
            assert _bytes_equal(a, b), f"frame {k}"
        _same_report(trk.gate_report(), g, f"frame {k} (the report still describes the frame)")
        again = mt.track_motion_tracker(trk, np.eye(4), T_C_B2)
        ul, ur = trk.undistorted()
        keep_l, keep_r = ~np.isin(l["id"], extra), ~np.isin(r["id"], extra)
        host = mt.track_motion(l["id"][keep_l], ul, r["id"][keep_r], ur, np.eye(4), T_C_B2)
        assert _bits(again) == _bits(host), f"frame {k}"
    for t in (trk, twin, mt):
        t.close()


# ---------------------------------------------------------------- 8. batch

def test_batch_of_handles_with_different_gates(gpu, seq):
    """Gates off, DROP_RIGHT, DROP_BOTH and DROP_BOTH at two pixels in one batch, on different
    sequences (one with a flat frame: empty lists); batch and single calls alternate."""
    cam, _ = _cams()["pinhole"]
    setup = [("h3", None, G.ONE_PIXEL), ("h3_from2", G.DROP_RIGHT, G.ONE_PIXEL), ("flatmid", G.DROP_BOTH, G.ONE_PIXEL),
             ("h3", G.DROP_BOTH, 2 * G.ONE_PIXEL)]
    twins = [_tracker(gpu, cam, m, e) for _, m, e in setup]
    ts = [_tracker(gpu, cam, m, e) for _, m, e in setup]
    tb = gpu.TrackerBatch(ts)
    rejected = [0] * 4
    for k in range(5):
        fr = [seq[s][k] for s, _, _ in setup]
        want = [t.process_frame(*f) for t, f in zip(twins, fr)]
        if k != 3:
            got = tb.process_frames([f[0] for f in fr], [f[1] for f in fr])
            assert tb.status == [0] * 4
        else:
            got = [t.process_frame(*f) for t, f in zip(ts, fr)]
        for i in range(4):
            what = f"frame {k} slot {i}"
            _same_lists(got[i], want[i], what)
            for a, b in zip(ts[i].undistorted(), twins[i].undistorted()):
                assert _bytes_equal(a, b), what
            (ca, ia, ea), (cb, ib, eb) = ts[i].gate_report(), twins[i].gate_report()
            assert ca == cb and np.array_equal(ia, ib) and _bytes_equal(ea, eb), what
            rejected[i] += ca.n_rejected
            if setup[i][1] is None:
                assert (ca.n_pairs, ca.n_rejected, ca.n_invalid) == (0, 0, 0)
        if k == 1:
            assert len(got[2][0]) == 0 and len(got[2][1]) == 0        # the flat frame
    assert rejected[0] == 0 and all(n > 20 for n in rejected[1:])
    tb.close()
    for t in ts + twins:
        t.close()


def test_small_streams_in_a_batch(gpu):
    """96 x 64 (6 to 10 pairs, 2 to 4 rejected per frame): nine gated streams against their single calls."""
    from rsvio import synthetic as S
    from rsvio.camera import Camera
    w, h = 96, 64
    cam = Camera.opencv5(120, 120, 48, 32)
    rendered = [[(l, G.h3(r)) for l, r in S.stereo_sequence(4, w, h, seed=s)] for s in (3, 4, 5)]
    modes = [G.DROP_BOTH, G.DROP_RIGHT, None]
    which = [(i % 3, modes[(i // 3) % 3]) for i in range(9)]
    twins = [_tracker(gpu, cam, m, w=w, h=h) for _, m in which]
    ts = [_tracker(gpu, cam, m, w=w, h=h) for _, m in which]
    tb = gpu.TrackerBatch(ts)
    total = 0
    for k in range(4):
        want = [t.process_frame(*rendered[q][k]) for t, (q, _) in zip(twins, which)]
        got = tb.process_frames([rendered[q][k][0] for q, _ in which], [rendered[q][k][1] for q, _ in which])
        for i in range(9):
            _same_lists(got[i], want[i], f"frame {k} slot {i}")
            (ca, ia, ea), (cb, ib, eb) = ts[i].gate_report(), twins[i].gate_report()
            assert ca == cb and np.array_equal(ia, ib) and _bytes_equal(ea, eb)
            total += ca.n_rejected
    assert total > 40
    tb.close()
    for t in ts + twins:
        t.close()


# ---------------------------------------------------------------- 9. refusals

def test_refusals_leave_the_handle_usable(gpu, seq):
    from rsvio import RsvioError, _lib
    from rsvio.tracker import StereoGate
    cam, conv = _cams()["pinhole"]
    lib = _lib.load()

    def refused(t, word, gate):
        with pytest.raises(RsvioError) as e:
            t.set_stereo_gate(gate)
        assert e.value.code == -1 and word in str(e.value), str(e.value)

    bare = _tracker(gpu)
    refused(bare, "cameras", StereoGate(1, G.ONE_PIXEL, G.RIG_T))
    bare.set_stereo_gate(None)                                           # off without cameras: fine
    bare.close()
    trk, twin = _tracker(gpu, cam), _tracker(gpu, cam, G.DROP_BOTH)
    for mode in (-1, 3):
        refused(trk, "mode", StereoGate(mode, G.ONE_PIXEL, G.RIG_T))
    for bad in (0.0, -1e-3, np.inf, np.nan):
        refused(trk, "max_error", StereoGate(1, bad, G.RIG_T))
    T = G.RIG_T.copy()
    T[2, 3] = np.inf
    refused(trk, "finite", StereoGate(1, G.ONE_PIXEL, T))
    T = G.RIG_T.copy()
    T[:3, 3] = 0
    refused(trk, "zero", StereoGate(1, G.ONE_PIXEL, T))
    T = G.RIG_T.copy()
    T[:3, :3] *= 1.001
    refused(trk, "orthonormal", StereoGate(1, G.ONE_PIXEL, T))
    frames = seq["h3"]
    trk.submit(*frames[0])
    refused(trk, "in flight", StereoGate(2, G.ONE_PIXEL, G.RIG_T))       # as rsvio_tracker_set_cameras
    l, r = trk.collect()
    assert trk.gate_report()[0].n_pairs == 0 and len(l) == len(r) > 30   # nothing was set: an ungated frame
    trk.remove_id(G.gate_lists(G.RIG_T, G.ONE_PIXEL, 2, conv, conv, l["id"], trk.undistorted()[0], r["id"],
                               trk.undistorted()[1]).rejected_ids)
    want = twin.process_frame(*frames[0])
    trk.set_stereo_gate(StereoGate(2, G.ONE_PIXEL, G.RIG_T))             # usable: from here on it is the twin
    with pytest.raises(RsvioError) as e:
        trk.set_cameras(None, None)                                      # refused while a gate is set
    assert e.value.code == -1 and "gate" in str(e.value)
    for k in (1, 2):
        got, want = trk.process_frame(*frames[k]), twin.process_frame(*frames[k])
        _same_lists(got, want, f"frame {k}")
    # the report's capacity rule, and zeros once the gate is off
    c, ids, err = trk.gate_report()
    assert c.n_rejected == 16
    small_i, small_e, n = np.zeros(5, np.uint64), np.zeros(5), C.c_size_t(0)
    rc = lib.rsvio_tracker_gate_report(trk._h, None, _lib.ptr(small_i), _lib.ptr(small_e), 5, C.byref(n))
    assert rc == CAPACITY and n.value == 16 and np.array_equal(small_i, ids[:5]) and _bytes_equal(small_e, err[:5])
    trk.set_stereo_gate(None)
    c, ids, err = trk.gate_report()
    assert (c.n_pairs, c.n_rejected, c.n_invalid, len(ids)) == (0, 0, 0, 0)
    trk.set_cameras(None, None)                                          # allowed again
    l, r = trk.process_frame(*frames[3])
    assert len(l) > 20
    trk.close()
    twin.close()


# ---------------------------------------------------------------- 10. Estimator

def _h3_from(frames, k0):
    return [(l, G.h3(r) if k >= k0 else r) for k, (l, r) in enumerate(frames)]


def test_estimator_with_a_gate_that_rejects_nothing_is_the_ungated_run(gpu, scene_stream):
    """max_error = 1: e <= 1 for unit bearings, so only invalid unprojections could go -- and there are none."""
    from rsvio.camera import Camera
    from rsvio.estimator import Estimator, StereoGateConfig
    s, win = scene_stream
    h, w = s.frames[0][0].shape
    cams = [Camera.opencv5(*p) for p in s.intrinsics]
    runs = []
    for gate in (None, StereoGateConfig(G.DROP_BOTH, 1.0)):
        est = Estimator(w, h, cams, s.T_B_Cl, s.T_B_Cr, window=win, stereo_gate=gate)
        runs.append(list(est.run(s.frames)))
        est.close()
    assert len(runs[0]) == len(s.frames) == 24
    for a, b in zip(*runs):
        assert a.n_gate_rejected is None and b.n_gate_rejected == 0
        assert (a.frame_id, a.is_keyframe, a.n_left, a.n_right, a.pnp_status, a.ba_status, a.pnp_iterations,
                a.ba_iterations, a.pnp_cost) == (b.frame_id, b.is_keyframe, b.n_left, b.n_right, b.pnp_status,
                                                 b.ba_status, b.pnp_iterations, b.ba_iterations, b.pnp_cost)
        assert np.array_equal(a.T_W_B, b.T_W_B)
    assert any(r.pnp_status is not None for r in runs[0]) and any(r.ba_status is not None for r in runs[0])


def test_estimator_gate_drops_displaced_right_observations(gpu, scene_stream):
    """H3 on the right images from frame 8 on, one-pixel threshold, DROP_BOTH (a rejected id frees its
    cell, so the displaced half keeps producing pairs to reject): rejections in every frame from
    that one on, no rejected id in a later right list, and the run finishes."""
    from rsvio.camera import Camera
    from rsvio.estimator import Estimator, StereoGateConfig
    s, win = scene_stream
    h, w = s.frames[0][0].shape
    cams = [Camera.opencv5(*p) for p in s.intrinsics]
    est = Estimator(w, h, cams, s.T_B_Cl, s.T_B_Cr, window=win,
                    stereo_gate=StereoGateConfig("drop_both", 1.0 / s.intrinsics[0][0]))
    trk = est.backend.tracker
    gone, results = set(), []
    for left, right in _h3_from(s.frames, 8):
        r = est.process_frame(left, right)
        right_ids = set(trk._out_r[:trk._n[1]]["id"].tolist())
        c, ids, _ = trk.gate_report()
        assert r.n_gate_rejected == c.n_rejected == len(ids) and r.n_right == len(right_ids)
        gone |= set(ids.tolist())
        assert not gone & right_ids
        results.append(r)
    est.close()
    assert len(results) == 24 and all(r.n_gate_rejected > 0 for r in results[8:])
    assert sum(r.n_gate_rejected for r in results[:8]) < results[8].n_gate_rejected
