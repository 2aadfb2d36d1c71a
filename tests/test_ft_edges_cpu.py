"""The feature_tracker/ crate variant's edge cases on the CPU oracle alone (no GPU).

Two things are pinned here so that test_ft_edges_gpu.py cannot pass vacuously:
  * ft_edges_reference.select_corners, a brute-force restatement of add_points, equals the oracle's
    add_points on every selection case -- ties, tracked features anywhere in u32, min_dist 0 .. 15;
  * every case of the GPU file takes the path it is there for: the tie fixture has ties inside
    min_dist, the LK cases keep valid and invalid tracks (or none at all), the dense sequence
    passes 1024 features, the box widths and copy levels are the ones the kernels branch on.
"""
import numpy as np
import pytest

import ft_edges_reference as R

f32 = np.float32
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0], f32)


def _corners(oracle, img, thr, md, blur, tracked=None):
    score = oracle.ft_shi_tomasi_score(img, blur)
    return score, oracle.ft_add_points(img, tracked, R.threshold_value(score, thr), md, blur)


# ---------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("case", R.selection_cases(), ids=lambda c: c[0])
def test_select_corners_equals_oracle(oracle, case):
    name, img, thr, md, blur, keys = case
    h, w = img.shape
    score, base = _corners(oracle, img, thr, md, blur)
    t = R.threshold_value(score, thr)
    assert np.array_equal(R.select_corners(score, None, t, md), base)
    if name.startswith("flat"):
        assert base.tolist() == ([[0, 0]] if md == 0 else [])
    if thr == "max":
        assert len(R.nms_candidates(score, t)) >= 1
    if thr == "above":
        assert len(base) == 0
    if len(keys) > 1:
        src = base if md <= R.VARIANT_MD else oracle.ft_add_points(img, None, t, R.VARIANT_MD, blur)
        assert len(src) >= 4
        variants = R.tracked_variants(src, h, w)
        for k in keys:
            ref = oracle.ft_add_points(img, variants[k], t, md, blur)
            assert np.array_equal(R.select_corners(score, variants[k], t, md), ref), k
            if k in ("on_corners", "half_off", "many") and md > 0 and len(base):
                assert len(ref) < len(base), k


def test_tie_fixture_has_ties(oracle):
    """Few distinct scores, one of them hundreds of times, and >= 100 equal-score candidate pairs
    within min_dist of each other; the corner counts of the fixture."""
    img = R.checkerboard(*R.TIE_SHAPE)
    for blur in R.TIE_BLURS:
        score = oracle.ft_shi_tomasi_score(img, blur)
        vals, counts = np.unique(score[score > 0], return_counts=True)
        assert len(vals) <= 1020 and counts.max() > 300, blur
        assert len(oracle.ft_add_points(img, None, 0.5, 3, blur)) == (165 if blur <= 2 else 96), blur
        cand = R.nms_candidates(score, 0.5)
        assert R.equal_score_pairs(cand, 15) >= 100, blur   # the squares are 8 px: none within 7


def test_height_cut_is_exercised(oracle):
    """A tracked feature above every corner and one below every corner; and results that depend on
    local_maxima's `height` being the largest candidate y rather than the image height -- with
    tracked features and without any."""
    differs = set()
    for name, img, thr, md, blur, keys in R.selection_cases():
        if name not in ("tie-md3-thr0.5", "tex-65x63", "wide-md7"):
            continue
        h, w = img.shape
        score, base = _corners(oracle, img, thr, md, blur)
        v = R.tracked_variants(base, h, w)
        assert v["below_all"][:, 1].max() <= base[:, 1].min()
        assert v["above_all"][:, 1].min() > base[:, 1].max()
        for k in keys:
            if not np.array_equal(R.select_corners(score, v[k], thr, md),
                                  R.select_corners(score, v[k], thr, md, window_to_image_height=True)):
                differs.add((name, k))
    assert {("tie-md3-thr0.5", "above_all"), ("tie-md3-thr0.5", "on_corners"), ("tex-65x63", "above_all"),
            ("wide-md7", "none")} <= differs


def test_round_sat_u32():
    cases = {np.nan: 0, -np.inf: 0, -1e10: 0, -0.5: 0, 0.49999997: 0, 0.5: 1, 1.5: 2, 2.5: 3, 8388607.5: 8388608,
             4294967040.0: 4294967040, 4294967296.0: R.U32_MAX, 1e10: R.U32_MAX, np.inf: R.U32_MAX}
    for v, want in cases.items():
        assert R.round_sat_u32(v) == want, v


# ---------------------------------------------------------------------------------- pyramid / score
def test_box_widths(oracle):
    for sigma, boxes in R.SCORE_BOXES.items():
        assert oracle.ft_boxes_for_gauss(sigma) == boxes, sigma


def test_copy_level_dims(oracle):
    for (h, w, L, ratio), dims in R.COPY_DIMS.items():
        assert oracle.ft_level_dims(w, h, L, ratio) == dims
        assert (h, w, L, ratio) in R.PYRAMID_CASES
    lv = oracle.ft_split_pyramid(oracle.ft_build_pyramid(R.noise(23, 17, 1), 4, 1.0), 17, 23, 4, 1.0)
    assert all(np.array_equal(lv[0], x) for x in lv[1:])   # a same-size Triangle resize is a copy


def test_same_size_level_is_a_copy_not_a_resize(oracle):
    """image's resize returns a copy at equal dimensions; a real resize clamps f32 samples to [0, 1]
    and sums from +0.  On an unblurred image with pixels outside [0, 1] and -0.0 the two differ:
    the same-size levels keep those pixels, the first resized level has none."""
    h, w, L, ratio = R.UNCLAMPED_CASES[1]
    assert oracle.ft_level_dims(w, h, L, ratio) == R.COPY_DIMS[(h, w, L, ratio)]
    img = R.unclamped(h, w)
    assert img.min() < -0.25 and img.max() > 1.25 and np.signbit(img[img == 0]).sum() >= 20
    lv = oracle.ft_split_pyramid(oracle.ft_build_pyramid(img, L, ratio, False), w, h, L, ratio)
    assert np.array_equal(lv[0].view(np.uint32), img.view(np.uint32))
    assert np.array_equal(lv[1].view(np.uint32), img.view(np.uint32))          # 17 x 23 again: a copy
    assert lv[2].min() >= 0.0 and lv[2].max() <= 1.0 and not np.signbit(lv[2]).any()   # 16 x 22: resized
    assert np.array_equal(lv[3].view(np.uint32), lv[2].view(np.uint32))
    clamped = np.clip(img, 0.0, 1.0) + f32(0.0)
    assert (lv[1].view(np.uint32) != clamped.view(np.uint32)).sum() >= 50          # what a {0, 1, 0}-tap resize gives


def test_tiny_levels(oracle):
    assert oracle.ft_level_dims(16, 16, 5)[-1] == (1, 1)
    assert oracle.ft_level_dims(64, 64, 7)[-1] == (1, 1)
    assert oracle.ft_level_dims(40, 33, 6)[3:] == [(5, 4), (3, 2), (1, 1)]
    assert oracle.ft_level_dims(16, 16, 7)[-1][0] == 0     # what the device refuses as too many levels
    ws = {c[1] for c in R.PYRAMID_CASES}
    hs = {c[0] for c in R.PYRAMID_CASES}
    assert {63, 64, 65, 127, 128, 129} <= ws and {7, 8, 9, 17} <= hs


# ----------------------------------------------------------------------------------------------- LK
def _lk_inputs(oracle, h, w, L, ratio, blur=True):
    a, b = R.pair(h, w, R.LK_SEED)
    p0 = oracle.ft_build_pyramid(a, L, ratio, blur)
    p1 = oracle.ft_build_pyramid(b, L, ratio, blur)
    corners = oracle.ft_add_points(p0[:w * h].reshape(h, w), None, R.TEX_THR, R.TEX_MD, R.TEX_BLUR).astype(f32)
    return p0, p1, np.concatenate([corners, R.border_ring(h, w)])


@pytest.mark.parametrize("case", R.LK_CASES, ids=str)
def test_lk_cases_track_and_fail(oracle, case):
    h, w, L, ratio, ssd, lssd = case
    p0, p1, xy = _lk_inputs(oracle, h, w, L, ratio)
    for cost, tracks in ((0, ssd), (1, lssd)):
        iso, ok = oracle.ft_track_points(p0, p1, w, h, xy, L, ratio, cost=cost)
        assert (~ok).sum() >= 10, (cost, ok.sum())
        if tracks:
            assert ok.sum() >= 20, (cost, ok.sum())
            assert len({tuple(r) for r in iso[ok].view(np.uint32).tolist()}) >= 20
        else:
            assert ok.sum() == 0, (cost, ok.sum())
        assert np.array_equal(iso[~ok], np.tile(IDENTITY, ((~ok).sum(), 1)))


def test_lk_all_fail(oracle):
    for h, w, L in R.LK_ALL_FAIL:
        p0, p1, xy = _lk_inputs(oracle, h, w, L, 2.0)
        assert len(xy) >= 80
        iso, ok = oracle.ft_track_points(p0, p1, w, h, xy, L, 2.0, cost=1)
        assert ok.sum() == 0, (h, w, L)
        assert np.array_equal(iso, np.tile(IDENTITY, (len(xy), 1)))


def test_lk_black_band(oracle):
    h, w, L = R.BAND_SHAPE
    a, b = R.black_band_pair(h, w, R.LK_SEED)
    p0, p1 = oracle.ft_build_pyramid(a, L, 2.0, False), oracle.ft_build_pyramid(b, L, 2.0, False)
    xy = R.band_points(h, w)
    inside = xy[:, 0] < w / 3 - 8
    assert inside.sum() >= 20 and (~inside).sum() >= 20
    _, lssd = oracle.ft_track_points(p0, p1, w, h, xy, L, 2.0, lam=0.1, cost=1)
    assert lssd[inside].sum() == 0 and lssd[~inside].sum() >= 10
    iso, ssd = oracle.ft_track_points(p0, p1, w, h, xy, L, 2.0, lam=0.1, cost=0)
    assert ssd[inside].sum() > inside.sum() // 2
    _, ssd0 = oracle.ft_track_points(p0, p1, w, h, xy, L, 2.0, lam=0.0, cost=0)
    assert ssd0[inside].sum() == 0 and ssd0[~inside].sum() >= 10   # inverse3 refuses H = 0


def test_lk_zero_iterations(oracle):
    h, w, L, ratio = R.LK_PARAM_SHAPE
    p0, p1, xy = _lk_inputs(oracle, h, w, L, ratio)
    xy = xy[:len(xy) - len(R.border_ring(h, w))]
    assert len(xy) >= 10
    for cost in (0, 1):
        iso, ok = oracle.ft_track_points(p0, p1, w, h, xy, L, ratio, max_iter=0, cost=cost)
        assert ok.all() and np.array_equal(iso, np.tile(IDENTITY, (len(xy), 1)))


def test_lk_parameters_matter(oracle):
    """max_iter and lambda change the transforms: the parameter sweep is no repetition of one case."""
    h, w, L, ratio = R.LK_PARAM_SHAPE
    p0, p1, xy = _lk_inputs(oracle, h, w, L, ratio)
    seen = set()
    for it in R.LK_ITERS:
        seen.add(oracle.ft_track_points(p0, p1, w, h, xy, L, ratio, max_iter=it)[0].tobytes())
    for lam in R.LK_LAMBDAS:
        seen.add(oracle.ft_track_points(p0, p1, w, h, xy, L, ratio, lam=lam)[0].tobytes())
    assert len(seen) == len(R.LK_ITERS) + len(R.LK_LAMBDAS)
    iso, ok = oracle.ft_track_points(p0, p1, w, h, R.lk_bad_points(h, w), L, ratio)
    assert not ok.any() and np.array_equal(iso, np.tile(IDENTITY, (len(iso), 1)))


# ------------------------------------------------------------------------------------------- handle
def test_dense_sequence_passes_1024(oracle):
    d = R.DENSE_CASE
    frames = R.sequence(d["h"], d["w"], 2, R.HANDLE_SEED)
    cfg = R.handle_config(oracle, d["nlevels"], detection_threshold=d["threshold"],
                          detection_min_dist=d["min_dist"], detection_blur=d["detection_blur"])
    t = oracle.FeatureTracker(d["w"], d["h"], cfg)
    ids0, _ = t.process_frame(frames[0])
    ids1, _ = t.process_frame(frames[1])
    assert len(ids0) > 1024
    assert (ids1 < len(ids0)).sum() > 1024


@pytest.mark.parametrize("cost", [0, 1])
def test_dying_sequence(oracle, cost):
    h, w, L, ratio = R.DYING_CASE
    t = oracle.FeatureTracker(w, h, R.handle_config(oracle, L, ratio, matching_cost=cost))
    seen = 0
    for k, img in enumerate(R.dying_sequence()):
        ids, _ = t.process_frame(img)
        if k == 1:
            assert (ids < seen).sum() >= 10
        if k == 2:   # every track died: fresh, consecutive ids only
            assert len(ids) >= 10 and np.array_equal(ids, seen + np.arange(len(ids), dtype=np.uint64))
        seen = max(seen, int(ids.max()) + 1)


@pytest.mark.parametrize("case", R.HANDLE_CASES, ids=str)
def test_handle_cases_track(oracle, case):
    h, w, L, ratio, blur = case
    for cost in (0, 1):
        t = oracle.FeatureTracker(w, h, R.handle_config(oracle, L, ratio, blur, matching_cost=cost))
        n0 = 0
        for k, img in enumerate(R.sequence(h, w, R.HANDLE_FRAMES, R.HANDLE_SEED)):
            ids, _ = t.process_frame(img)
            if k == 0:
                n0 = len(ids)
                assert n0 >= 20
        kept = (ids < n0).sum()
        assert len(ids) > kept        # new corners in the last frame
        if not (cost == 1 and L >= 4 and ratio == 2.0):
            assert kept >= 5, (cost, kept)   # tracks of frame 0 alive after four frames
