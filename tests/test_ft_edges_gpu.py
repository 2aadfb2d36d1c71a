"""GPU parity of the feature_tracker/ crate variant at its edges: small and ragged shapes, copy levels,
box-blur radii on the kernel variants' boundaries, score ties, tracked features anywhere in u32,
LK parameter extremes and zero-mean LSSD patches, and the handle's refusals -- every case against
the CPU oracle bit for bit (uint32 views, integer lists), through the C ABI.

The cases and inputs are tests/ft_edges_reference.py's; test_ft_edges_cpu.py shows on the oracle
alone that each case takes the path it is here for, and that select_corners (the brute-force
restatement the selection results are also compared with) equals the oracle.
"""
import ctypes as C

import numpy as np
import pytest

import ft_edges_reference as R

pytestmark = pytest.mark.gpu
f32 = np.float32
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0], f32)
INVALID_ARG, CAPACITY = -1, -4


@pytest.fixture(scope="module")
def ftg(gpu):
    from rsvio import ft
    return ft


@pytest.fixture(scope="module")
def lib(gpu):
    from rsvio import _lib
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def refused(fn, *a, **kw):
    """The RsvioError code of a call that must be refused."""
    from rsvio import RsvioError
    with pytest.raises(RsvioError) as e:
        fn(*a, **kw)
    return e.value.code


# ------------------------------------------------------------------------------------------ pyramid
@pytest.mark.parametrize("case", R.PYRAMID_CASES, ids=str)
def test_pyramid_shapes(ftg, oracle, case):
    h, w, L, ratio = case
    img = R.noise(h, w, L)
    for blur in (True, False):
        ref = oracle.ft_build_pyramid(img, L, ratio, blur)
        out = ftg.build_image_pyramid(img, L, ratio, blur)
        assert ftg.level_dims(w, h, L, ratio) == oracle.ft_level_dims(w, h, L, ratio)
        assert out.shape == ref.shape
        assert np.array_equal(bits(out), bits(ref)), blur


@pytest.mark.parametrize("case", R.UNCLAMPED_CASES, ids=str)
def test_pyramid_unclamped_input(ftg, oracle, case):
    """Unblurred, pixels outside [0, 1] and -0.0: level 0 and its same-size copies keep them (the
    reference's resize returns a copy at equal dimensions), a resized level is clamped."""
    h, w, L, ratio = case
    img = R.unclamped(h, w)
    ref = oracle.ft_build_pyramid(img, L, ratio, False)
    assert np.array_equal(bits(ftg.build_image_pyramid(img, L, ratio, False)), bits(ref))
    assert np.array_equal(bits(ftg.build_image_pyramid(img, L, ratio, True)),
                          bits(oracle.ft_build_pyramid(img, L, ratio, True)))


@pytest.mark.parametrize("sigma", R.PYRAMID_SIGMAS)
def test_pyramid_blur_sigma(ftg, oracle, sigma):
    """sigma <= 0 falls back to 1; 0.5 has 3-tap rows, 5.0 a 21-tap support (the tile span grows)."""
    for h, w, L, ratio in R.PYRAMID_SIGMA_SHAPES:
        img = R.noise(h, w, 3)
        ref = oracle.ft_build_pyramid(img, L, ratio, True, sigma)
        assert np.array_equal(bits(ftg.build_image_pyramid(img, L, ratio, True, sigma)), bits(ref)), (h, w)
        if sigma <= 0:
            assert np.array_equal(bits(ref), bits(oracle.ft_build_pyramid(img, L, ratio, True, 1.0)))


@pytest.mark.parametrize("case", R.PYRAMID_REFUSED, ids=str)
def test_pyramid_refusals(lib, case):
    """Decided on the host before any launch: an error code, and nothing written."""
    h, w, L, ratio = case
    img = np.zeros((h, w), f32)
    out = np.full(4096, 7.0, f32)
    assert lib.rsvio_ft_build_pyramid(img.ctypes.data, w, h, L, ratio, 1, C.c_float(2.0), out.ctypes.data) == INVALID_ARG
    assert (out == 7.0).all()
    assert lib.rsvio_ft_pyramid_floats(w, h, L, ratio) == 0


# -------------------------------------------------------------------------------------------- score
@pytest.mark.parametrize("shape", R.SCORE_SHAPES, ids=str)
def test_score_shapes_and_radii(ftg, oracle, shape):
    """r = 0 (sigma 0.5); r = 31, 31, 32 (sigma 32: both tiled variants in one call); r = 63, 63, 64
    (sigma 64: the 3-segment tiles and the any-radius kernel); widths of one chunk, of whole chunks
    and ragged ones; on 16 x 16 a radius larger than the row."""
    h, w = shape
    img = R.noise(h, w, 11)
    for blur in R.SCORE_BLURS:
        assert np.array_equal(bits(ftg.shi_tomasi_score(img, blur)), bits(oracle.ft_shi_tomasi_score(img, blur))), blur


@pytest.mark.parametrize("blur", R.TIE_BLURS)
def test_score_tie_fixture(ftg, oracle, blur):
    img = R.checkerboard(*R.TIE_SHAPE)
    assert np.array_equal(bits(ftg.shi_tomasi_score(img, blur)), bits(oracle.ft_shi_tomasi_score(img, blur)))


# ---------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("case", R.selection_cases(), ids=lambda c: c[0])
def test_selection(ftg, oracle, case):
    name, img, thr, md, blur, keys = case
    h, w = img.shape
    score = oracle.ft_shi_tomasi_score(img, blur)
    t = R.threshold_value(score, thr)
    base = oracle.ft_add_points(img, None, t, md, blur)
    src = base if md <= R.VARIANT_MD else oracle.ft_add_points(img, None, t, R.VARIANT_MD, blur)
    variants = R.tracked_variants(src, h, w) if len(keys) > 1 else {"none": None}
    brute = max(h, w) <= 256   # the O(n^2) restatement: not on the 2048-wide cases
    for k in keys:
        out = ftg.add_points(img, variants[k], t, md, blur)
        assert out.dtype == np.uint32
        assert np.array_equal(out, oracle.ft_add_points(img, variants[k], t, md, blur)), k
        if brute:
            assert np.array_equal(out, R.select_corners(score, variants[k], t, md)), k


def _add_points_raw(lib, img, thr, md, blur, cap):
    h, w = img.shape
    out = np.full((max(cap, 1) + 4, 2), 0xABCDABCD, np.uint32)
    n = C.c_int32(-1)
    code = lib.rsvio_ft_add_points(img.ctypes.data, w, h, None, 0, C.c_float(thr), md, C.c_float(blur),
                                   out.ctypes.data, cap, C.byref(n))
    return code, n.value, out


def test_add_points_capacity(lib, oracle):
    """cap == the corner count is enough; one less is RSVIO_ERR_CAPACITY with the full count, the
    first cap corners written and nothing past them."""
    img = R.tex(63, 65, 5)
    ref = oracle.ft_add_points(img, None, R.TEX_THR, R.TEX_MD, R.TEX_BLUR)
    k = len(ref)
    assert k >= 8
    code, n, out = _add_points_raw(lib, img, R.TEX_THR, R.TEX_MD, R.TEX_BLUR, k)
    assert (code, n) == (0, k) and np.array_equal(out[:k], ref) and (out[k:] == 0xABCDABCD).all()
    code, n, out = _add_points_raw(lib, img, R.TEX_THR, R.TEX_MD, R.TEX_BLUR, k - 1)
    assert (code, n) == (CAPACITY, k) and np.array_equal(out[:k - 1], ref[:k - 1]) and (out[k - 1:] == 0xABCDABCD).all()


def test_add_points_refusals(ftg):
    img = R.tex(63, 65, 5)
    assert refused(ftg.add_points, img, None, 0.05, -1) == INVALID_ARG
    assert refused(ftg.add_points, img, None, 0.05, 32) == INVALID_ARG            # 2 md >= min(w, h)
    assert refused(ftg.add_points, R.noise(16, 2050, 1), None, 0.05, 1) == INVALID_ARG   # 1025 NMS blocks a row
    assert refused(ftg.shi_tomasi_score, R.noise(3, 16, 1)) == INVALID_ARG


# ----------------------------------------------------------------------------------------------- LK
def _lk_inputs(oracle, h, w, L, ratio):
    a, b = R.pair(h, w, R.LK_SEED)
    p0 = oracle.ft_build_pyramid(a, L, ratio)
    p1 = oracle.ft_build_pyramid(b, L, ratio)
    corners = oracle.ft_add_points(p0[:w * h].reshape(h, w), None, R.TEX_THR, R.TEX_MD, R.TEX_BLUR).astype(f32)
    return p0, p1, np.concatenate([corners, R.border_ring(h, w)])


def _lk_equal(ftg, oracle, p0, p1, w, h, xy, L, ratio, max_iter=25, lam=0.1, cost=0):
    ref_iso, ref_ok = oracle.ft_track_points(p0, p1, w, h, xy, L, ratio, max_iter, lam, cost)
    iso, ok = ftg.track_points(p0, p1, w, h, xy, L, ratio, max_iter, lam, cost)
    assert np.array_equal(ok, ref_ok), (ok.sum(), ref_ok.sum())
    assert np.array_equal(bits(iso), bits(ref_iso))
    return iso, ok


@pytest.mark.parametrize("cost", [0, 1])
@pytest.mark.parametrize("case", R.LK_CASES, ids=str)
def test_lk_shapes(ftg, oracle, case, cost):
    """Corners plus the border ring at 1, 3, 4 and 5 levels, ratios 1.0, 1.3 and 2.0."""
    h, w, L, ratio = case[:4]
    p0, p1, xy = _lk_inputs(oracle, h, w, L, ratio)
    _lk_equal(ftg, oracle, p0, p1, w, h, xy, L, ratio, cost=cost)


@pytest.mark.parametrize("cost", [0, 1])
def test_lk_iterations_and_lambda(ftg, oracle, cost):
    h, w, L, ratio = R.LK_PARAM_SHAPE
    p0, p1, xy = _lk_inputs(oracle, h, w, L, ratio)
    for it in R.LK_ITERS:
        iso, ok = _lk_equal(ftg, oracle, p0, p1, w, h, xy, L, ratio, max_iter=it, cost=cost)
        if it == 0:   # the loop never runs: whatever builds a patch at every level is valid, unmoved
            assert ok.sum() >= 20 and np.array_equal(iso, np.tile(IDENTITY, (len(xy), 1)))
    for lam in R.LK_LAMBDAS:
        _lk_equal(ftg, oracle, p0, p1, w, h, xy, L, ratio, lam=lam, cost=cost)


@pytest.mark.parametrize("cost", [0, 1])
@pytest.mark.parametrize("lam", [0.1, 0.0])
def test_lk_black_band(ftg, oracle, cost, lam):
    """Patches of mean 0: LSSD's 0 / 0 (invalid, identity), SSD's H = lambda I (valid) or H = 0
    (inverse3 refuses)."""
    h, w, L = R.BAND_SHAPE
    a, b = R.black_band_pair(h, w, R.LK_SEED)
    p0, p1 = oracle.ft_build_pyramid(a, L, 2.0, False), oracle.ft_build_pyramid(b, L, 2.0, False)
    xy = R.band_points(h, w)
    iso, ok = _lk_equal(ftg, oracle, p0, p1, w, h, xy, L, 2.0, lam=lam, cost=cost)
    inside = xy[:, 0] < w / 3 - 8
    if cost == 1 or lam == 0.0:
        assert not ok[inside].any() and np.array_equal(iso[inside], np.tile(IDENTITY, (inside.sum(), 1)))


@pytest.mark.parametrize("case", R.LK_ALL_FAIL, ids=str)
def test_lk_undersized_levels(ftg, oracle, case):
    """Levels smaller than the 15 x 15 pattern, down to 1 x 1: every lane misses."""
    h, w, L = case
    p0, p1, xy = _lk_inputs(oracle, h, w, L, 2.0)
    for cost in (0, 1):
        iso, ok = _lk_equal(ftg, oracle, p0, p1, w, h, xy, L, 2.0, cost=cost)
        if cost == 1:
            assert not ok.any() and np.array_equal(iso, np.tile(IDENTITY, (len(xy), 1)))


@pytest.mark.parametrize("cost", [0, 1])
def test_lk_bad_positions(ftg, oracle, cost):
    h, w, L, ratio = R.LK_PARAM_SHAPE
    p0, p1, _ = _lk_inputs(oracle, h, w, L, ratio)
    xy = R.lk_bad_points(h, w)
    iso, ok = _lk_equal(ftg, oracle, p0, p1, w, h, xy, L, ratio, cost=cost)
    assert not ok.any() and np.array_equal(iso, np.tile(IDENTITY, (len(xy), 1)))


def test_lk_refusals(ftg, lib):
    h, w, L, ratio = R.LK_PARAM_SHAPE
    p = np.zeros(ftg.pyramid_floats(w, h, L, ratio), f32)
    xy = np.array([[20.0, 20.0]], f32)
    assert refused(ftg.track_points, p, p, w, h, xy, L, ratio, max_iteration=-1) == INVALID_ARG
    assert refused(ftg.track_points, p, p, w, h, xy, L, ratio, matching_cost=2) == INVALID_ARG
    assert refused(ftg.track_points, p, p, w, h, xy, L, ratio, matching_cost=-1) == INVALID_ARG
    iso, ok = np.full((1, 4), 7.0, f32), np.full(1, 7, np.uint8)
    assert lib.rsvio_ft_track_points(p.ctypes.data, p.ctypes.data, w, h, L, ratio, xy.ctypes.data, -1, 25,
                                     C.c_float(0.1), 0, iso.ctypes.data, ok.ctypes.data) == INVALID_ARG
    assert (iso == 7.0).all() and ok[0] == 7


# ------------------------------------------------------------------------------------------- handle
def _same_frame(f, rid, rxy):
    return np.array_equal(f["feature_id"], rid) and np.array_equal(bits(np.stack([f["x"], f["y"]], 1)), bits(rxy))


def _twin(ftg, oracle, h, w, cost=0, max_features=8192, **cfg):
    ref = oracle.FeatureTracker(w, h, R.handle_config(oracle, matching_cost=cost, **cfg))
    t = ftg.FeatureTracker(w, h, R.handle_config(ftg, **cfg), matching_cost=cost, max_features=max_features)
    return ref, t


@pytest.mark.parametrize("cost", [0, 1])
@pytest.mark.parametrize("case", R.HANDLE_CASES, ids=str)
def test_handle_shapes(ftg, oracle, case, cost):
    h, w, L, ratio, blur = case
    ref, t = _twin(ftg, oracle, h, w, cost, nlevels=L, ratio=ratio, blur=blur)
    assert refused(t.get_pyramid) == INVALID_ARG                 # no frame yet
    for k, img in enumerate(R.sequence(h, w, R.HANDLE_FRAMES, R.HANDLE_SEED)):
        assert _same_frame(t.process(img), *ref.process_frame(img)), k
        lv = t.get_pyramid()
        ref_lv = oracle.ft_split_pyramid(oracle.ft_build_pyramid(img, L, ratio, blur), w, h, L, ratio)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(lv, ref_lv)), k
    t.close()


def test_handle_dense(ftg, oracle):
    """More than 1024 tracked features: ft_assemble_kernel's lanes own more than one each."""
    d = R.DENSE_CASE
    h, w = d["h"], d["w"]
    ref, t = _twin(ftg, oracle, h, w, nlevels=d["nlevels"], detection_threshold=d["threshold"],
                   detection_min_dist=d["min_dist"], detection_blur=d["detection_blur"])
    n0 = 0
    for k, img in enumerate(R.sequence(h, w, 3, R.HANDLE_SEED)):
        rid, rxy = ref.process_frame(img)
        assert _same_frame(t.process(img), rid, rxy), k
        if k == 0:
            n0 = len(rid)
        elif k == 1:
            assert (rid < n0).sum() > 1024
    t.close()


@pytest.mark.parametrize("cost", [0, 1])
def test_handle_every_track_dies(ftg, oracle, cost):
    h, w, L, ratio = R.DYING_CASE
    ref, t = _twin(ftg, oracle, h, w, cost, nlevels=L, ratio=ratio)
    seen = 0
    for k, img in enumerate(R.dying_sequence()):
        f = t.process(img)
        assert _same_frame(f, *ref.process_frame(img)), k
        if k == 2:
            assert np.array_equal(f["feature_id"], seen + np.arange(len(f), dtype=np.uint64))
        seen = max(seen, int(f["feature_id"].max()) + 1)
    t.close()


def test_handle_device_image(ftg, oracle):
    """process_frame_device on a torch tensor equals process on a twin handle."""
    import torch
    h, w, L, ratio, blur = R.HANDLE_CASES[1]
    _, a = _twin(ftg, oracle, h, w, nlevels=L, ratio=ratio, blur=blur)
    _, b = _twin(ftg, oracle, h, w, nlevels=L, ratio=ratio, blur=blur)
    for k, img in enumerate(R.sequence(h, w, 3, R.HANDLE_SEED)):
        d = torch.from_numpy(np.array(img)).cuda()
        torch.cuda.synchronize()
        n = b.process_frame_device(d.data_ptr())
        fa, fb = a.process(img), b.features()
        assert n == len(fa) and len(fa) >= 20 and fa.tobytes() == fb.tobytes(), k
    a.close()
    b.close()


def _process_raw(lib, t, img, stride):
    n = C.c_size_t(0)
    code = lib.rsvio_ft_process_frame(t._h, img.ctypes.data, stride, t._out.ctypes.data, t.cap, C.byref(n))
    return code, t._out[:n.value].copy()


def test_handle_stride(ftg, oracle, lib):
    """A padded host image (stride = width + 5) equals the contiguous call; a stride below the
    width is refused and leaves the handle as it was."""
    h, w, L, ratio, blur = R.HANDLE_CASES[0]
    ref, t = _twin(ftg, oracle, h, w, nlevels=L, ratio=ratio, blur=blur)
    for k, img in enumerate(R.sequence(h, w, 3, R.HANDLE_SEED)):
        pad = np.full((h, w + 5), np.nan, f32)
        pad[:, :w] = img
        if k == 1:
            assert _process_raw(lib, t, pad, w - 1)[0] == INVALID_ARG
        code, f = _process_raw(lib, t, pad, w + 5)
        assert code == 0 and _same_frame(f, *ref.process_frame(img)), k
    t.close()


def test_handle_pyramid_buffer(ftg, oracle, lib):
    h, w, L, ratio, blur = R.HANDLE_CASES[0]
    _, t = _twin(ftg, oracle, h, w, nlevels=L, ratio=ratio, blur=blur)
    n = ftg.pyramid_floats(w, h, L, ratio)
    buf = np.full(n, 7.0, f32)
    assert lib.rsvio_ft_get_pyramid(t._h, buf.ctypes.data, n) == INVALID_ARG      # before any frame
    img = R.sequence(h, w, 2, R.HANDLE_SEED)[0]
    t.process(img)
    assert lib.rsvio_ft_get_pyramid(t._h, buf.ctypes.data, n - 1) == CAPACITY     # one float short
    assert (buf == 7.0).all()
    assert lib.rsvio_ft_get_pyramid(t._h, buf.ctypes.data, n) == 0
    assert np.array_equal(bits(buf), bits(oracle.ft_build_pyramid(img, L, ratio, blur)))
    t.close()


def test_handle_max_features(ftg, oracle, lib):
    """A list that fills max_features exactly is complete; one slot less is RSVIO_ERR_CAPACITY, after
    which the handle still takes frames; a twin with room goes on matching the oracle."""
    h, w, L, ratio, blur = R.HANDLE_CASES[0]
    frames = R.sequence(h, w, 3, R.HANDLE_SEED)
    ref, roomy = _twin(ftg, oracle, h, w, nlevels=L, ratio=ratio, blur=blur)
    rid, rxy = ref.process_frame(frames[0])
    n0 = len(rid)
    assert n0 >= 20
    _, exact = _twin(ftg, oracle, h, w, max_features=n0, nlevels=L, ratio=ratio, blur=blur)
    _, short = _twin(ftg, oracle, h, w, max_features=n0 - 1, nlevels=L, ratio=ratio, blur=blur)
    assert _same_frame(exact.process(frames[0]), rid, rxy)
    assert _same_frame(roomy.process(frames[0]), rid, rxy)
    code, f = _process_raw(lib, short, np.array(frames[0]), w)
    assert code == CAPACITY and _same_frame(f, rid[:n0 - 1], rxy[:n0 - 1])
    code, f = _process_raw(lib, short, np.array(frames[1]), w)
    assert code in (0, CAPACITY) and len(f) <= n0 - 1
    assert np.isfinite(f["x"]).all() and len(set(f["feature_id"].tolist())) == len(f)
    for k in (1, 2):
        assert _same_frame(roomy.process(frames[k]), *ref.process_frame(frames[k])), k
    for t in (exact, short, roomy):
        t.close()


@pytest.mark.parametrize("bad", [dict(width=15), dict(height=15), dict(nlevels=0), dict(nlevels=9), dict(ratio=0.0),
                                 dict(matching_cost=2), dict(detection_min_dist=32), dict(max_features=-1),
                                 dict(optical_flow_max_iter=-1)], ids=str)
def test_create_refusals(ftg, bad):
    args = dict(width=64, height=64, matching_cost=0, max_features=64)
    cfg = dict(nlevels=2, ratio=2.0, detection_min_dist=2)
    for k, v in bad.items():
        (args if k in args else cfg)[k] = v
    c = R.handle_config(ftg, **cfg)
    assert refused(ftg.FeatureTracker, args["width"], args["height"], c, args["matching_cost"], 0,
                   args["max_features"]) == INVALID_ARG
    ok = ftg.FeatureTracker(64, 64, R.handle_config(ftg, nlevels=2, detection_min_dist=31), 0, 0, 64)   # 2 md < 64
    ok.close()
