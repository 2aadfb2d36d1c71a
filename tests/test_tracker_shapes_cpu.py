"""The conditions under which test_tracker_shapes_gpu.py means something, evaluated on the CPU oracle:
an input that drifts into triviality (nothing tracked, everything tracked, no corner, a parameter
that changes nothing, a shape that no longer takes the path it was chosen for) fails here, without
a device.  The inputs and case tables are tests/tracker_shapes_reference.py's.
"""
import numpy as np
import pytest

import tracker_shapes_reference as R


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------- inputs
def test_texture_has_gradient_at_every_level(oracle):
    """texture: u8 over the full range, and still not flat at level 7 (noise alone is: 127 / 128)."""
    for h, w in R.DIRECT_SHAPES:
        img = R.texture(h, w, 3)
        assert img.dtype == np.uint8 and img.shape == (h, w) and img.min() == 0 and img.max() == 255
        pyr = oracle.build_pyramid(img, 8)
        top = pyr[oracle.pyramid_bytes(w, h, 7):]
        assert len(top) == (h >> 7) * (w >> 7) and len(np.unique(top)) >= 3
        flat = oracle.build_pyramid(R.noise_image(h, w, 8), 8)[oracle.pyramid_bytes(w, h, 7):]
        assert set(np.unique(flat).tolist()) <= {126, 127, 128, 129}


def test_shifted_frames_move_as_documented():
    fr = R.shifted_frames(64, 80, 3, 5, 0)
    (l0, r0), (l2, _) = fr[0], fr[2]
    assert np.array_equal(l0[:, 4:], r0[:, :-4])            # the right image: 4 px disparity
    assert np.array_equal(l0[:-2, 4:], l2[2:, :-4])         # frame 2: content moved by (-4, +2)
    a, b = R.shifted_pair(64, 80, 5)
    assert np.array_equal(a[:-3, 2:], b[3:, :-2])           # the pair: (-2, +3)
    n0, n1 = R.shifted_frames(64, 80, 2, 5, 6)[0]
    assert not np.array_equal(n0[:, 4:], n1[:, :-4])        # noise is per image
    assert 0 < np.abs(n0.astype(int) - R.shifted_frames(64, 80, 2, 5, 0)[0][0].astype(int)).max() <= 6


# ------------------------------------------------------------------------------------- pyramid plan
def test_plan_direct_masks():
    """The plan's arithmetic in numpy: the shapes chosen for the HBM-tap path take it at level 7 and
    only there, the others stay on the LDS path, and the launch never asks for more than 64 KiB."""
    for h, w, L, direct in R.PYRAMID_CASES:
        p = R.pyramid_plan(w, h, L)
        assert p["lds_bytes"] <= 65536, (h, w, L)
        if direct is not None:
            assert p["direct"] == direct, (h, w, L)
    for h, w in R.DIRECT_SHAPES:
        assert R.pyramid_plan(w, h, 8)["direct"] == 1 << 7
    # the footprints (strip, vert) the shapes were chosen by
    assert R.pyramid_plan(384, 384, 8)["foot"][7] == (65536, 1024)
    assert R.pyramid_plan(416, 400, 8)["foot"][7] == (75040, 1112)
    assert R.pyramid_plan(1000, 600, 8)["foot"][7] == (87600, 1148)
    assert R.pyramid_plan(256, 256, 8)["foot"][7] == (36864, 768)
    assert R.pyramid_plan(447, 383, 7)["foot"][6] == (35340, 900)
    assert (130 >> 6, 200 >> 6) == (2, 3)
    # levels 6 and 7 are built output by output
    p = R.pyramid_plan(1000, 600, 8)
    assert p["tile_w"][7] == p["tile_h"][7] == 1 and p["tile_h"][6] == 1
    # the frame pipeline's deepest shapes: L = 8 reads level 7 from HBM, L = 7 does not
    assert R.pyramid_plan(1920, 1664, 8)["direct"] == 1 << 7
    assert R.pyramid_plan(960, 832, 7)["direct"] == 0


def test_plan_readback_abi():
    """rsvio_dbg_pyramid_plan is exported and refuses bad arguments before it needs a device."""
    import ctypes as C

    from rsvio import _lib
    lib = _lib.load()
    tw, th = np.zeros(8, np.int32), np.zeros(8, np.int32)
    d, n = C.c_uint32(0), C.c_uint64(0)
    assert lib.rsvio_dbg_pyramid_plan(64, 64, 3, None, _lib.ptr(th), C.byref(d), C.byref(n)) == -1
    assert lib.rsvio_dbg_pyramid_plan(64, 64, 9, _lib.ptr(tw), _lib.ptr(th), C.byref(d), C.byref(n)) == -1
    assert lib.rsvio_dbg_pyramid_plan(8, 64, 3, _lib.ptr(tw), _lib.ptr(th), C.byref(d), C.byref(n)) == -1


def test_plan_taps_fit_the_table():
    """max_taps = ceil(2 max_ratio) + 4 holds every tap count, also for the non-integer ratios
    (600 / 4 = 150 and 1000 / 7 = 142.86) of the deepest levels."""
    for h, w, L, _ in R.PYRAMID_CASES:
        worst, max_ratio = 0, np.float32(1.0)
        for i in range(1, L):
            for n in (w, h):
                worst = max(worst, int(R.taps(n, n >> i)[1].max()))
                max_ratio = max(max_ratio, np.float32(n) / np.float32(n >> i))
        assert worst <= int(np.ceil(np.float32(2.0) * max_ratio)) + 4, (h, w, L)
    assert np.float32(1000) / np.float32(7) > 142.8 and 600 / 4 == 150


def test_packed_images_are_unaligned():
    """Packed mode: image 1 onward (and its pyramid) starts off a 16-byte boundary."""
    for n, h, w, L in R.PACKED_CASES:
        assert (h * w) % 16 != 0
    assert 61 * 97 == 5917


def test_pyramid_prefix(oracle):
    """A pyramid of L levels is the head of a deeper one (every level comes from level 0)."""
    img = R.texture(130, 200, 1)
    deep = oracle.build_pyramid(img, 7)
    for L in (1, 3, 5):
        assert np.array_equal(oracle.build_pyramid(img, L), deep[:oracle.pyramid_bytes(200, 130, L)])


# ---------------------------------------------------------------------------------------------- LK
@pytest.fixture(scope="module")
def depth(oracle):
    h, w = R.DEPTH_SHAPE
    a, b = R.shifted_pair(h, w, 11)
    return oracle.build_pyramid(a, 8), oracle.build_pyramid(b, 8), R.lk_states(h, w, 96, 5)


def test_lk_every_depth_condition(oracle, depth):
    """Per L the oracle keeps between 24 and 92 of the 96 states, none of the 8 outside ones."""
    h, w = R.DEPTH_SHAPE
    p0, p1, aff = depth
    counts = []
    for L in range(1, 9):
        nb = oracle.pyramid_bytes(w, h, L)
        ra, rv = oracle.track_points(p0[:nb], p1[:nb], w, h, L, aff)
        counts.append(int(rv.sum()))
        assert 24 <= counts[-1] <= 92, (L, counts)
        assert not rv[-8:].any()
        # (a few tracks may settle on a look-alike; most land on the true displacement)
        assert np.median(np.abs(ra[rv][:, 4:6] - aff[rv][:, 4:6] - np.array(R.DEPTH_SHIFT, np.float32))) < 0.1
    print("oracle valid per L:", counts)


def test_lk_every_depth_seeded_condition(depth):
    """The seeded reference keeps at least 24 states per L, some from each kind of seed (exact,
    1.5 px off, NaN)."""
    import seeded_tracking_reference as SR
    from oracle import oracle as O
    h, w = R.DEPTH_SHAPE
    p0, p1, aff = depth
    seeds = R.lk_seeds(aff, R.DEPTH_SHIFT)
    assert np.isnan(seeds[2::3]).all() and np.isfinite(seeds[0::3]).all() and np.isfinite(seeds[1::3]).all()
    counts = []
    for L in range(1, 9):
        nb = O.pyramid_bytes(w, h, L)
        _, rv = SR.track_points_seeded(p0[:nb], p1[:nb], w, h, L, aff, seeds)
        counts.append(int(rv.sum()))
        assert 24 <= counts[-1] <= 92 and all(rv[k::3].any() for k in range(3)), (L, counts)
    print("seeded reference valid per L:", counts)


def test_lk_undersized_all_invalid(oracle):
    """A pyramid whose top level is 1 x 1, 3 x 3 or 5 x 6 (no room for 27 of the 52 pattern points)
    rejects every state and hands the input back; the mixed companion keeps some."""
    for h, w, L in R.UNDERSIZED_CASES:
        assert (h >> (L - 1), w >> (L - 1)) in ((1, 1), (3, 3), (5, 6))
        a, b = R.shifted_pair(h, w, 20 + L)
        aff = R.lk_states(h, w, 64, 6)
        ra, rv = oracle.track_points(oracle.build_pyramid(a, L), oracle.build_pyramid(b, L), w, h, L, aff)
        assert not rv.any(), (h, w, L)
        assert np.array_equal(_bits(ra), _bits(aff)), (h, w, L)
    h, w, L = R.MIXED_CASE
    a, b = R.shifted_pair(h, w, 20 + L)
    _, rv = oracle.track_points(oracle.build_pyramid(a, L), oracle.build_pyramid(b, L), w, h, L,
                                R.lk_states(h, w, 64, 6))
    assert 8 <= rv.sum() <= 56
    print("mixed companion valid:", int(rv.sum()))


def test_lk_one_pixel_level_reads_nothing_outside(oracle):
    """A far-away state on a pyramid with a 1 x 1 top level: the wrapped `width - 2` used to pass
    its in-bound test and index the level at 6e7."""
    a, b = R.shifted_pair(20, 20, 25)
    aff = R.identity_states([[1e9, 5.0], [5.0, 3e9], [40.0, 40.0]])
    ra, rv = oracle.track_points(oracle.build_pyramid(a, 5), oracle.build_pyramid(b, 5), 20, 20, 5, aff)
    assert not rv.any() and np.array_equal(_bits(ra), _bits(aff))


def test_lk_parameter_edges_condition(oracle):
    """Every (max_iterations, thresh) but (20, 0.01) and (100, 0.01) changes the oracle's output on
    at least half of the states the default parameters keep: the parameter was exercised."""
    h, w, L = R.EDGE_SHAPE
    a, b = R.edge_pair()
    p0, p1 = oracle.build_pyramid(a, L), oracle.build_pyramid(b, L)
    aff = R.lk_states(h, w, 96, 8)
    da, dv = oracle.track_points(p0, p1, w, h, L, aff)
    assert dv.sum() >= 48
    seen = []
    for it, th in R.EDGE_COMBOS:
        ra, rv = oracle.track_points(p0, p1, w, h, L, aff, it, th)
        differ = ((rv != dv) | (_bits(ra) != _bits(da)).any(1))[dv]
        seen.append(int(differ.sum()))
        if (it, th) not in R.EDGE_SAME_AS_DEFAULT:
            assert 2 * differ.sum() >= dv.sum(), (it, th, int(differ.sum()), int(dv.sum()))
    print("default valid:", int(dv.sum()), "differing:", min(seen), "..", max(seen))


# -------------------------------------------------------------------------------------------- FAST
def test_fast_conditions(oracle):
    counts = []
    for h, w, g in R.FAST_CASES:
        img = R.fast_image(h, w, g)
        xy, _ = oracle.detect_key_points(img, g)
        xy2, _ = oracle.detect_key_points(img, g, R.fast_existing(h, w, g, xy))
        counts.append((len(xy), len(xy2)))
        if (h, w, g) == R.FAST_EMPTY:
            assert len(xy) == 0 and len(xy2) == 0     # no candidate survives the 19 px border
        else:
            assert len(xy) >= 1 and len(xy2) < len(xy), (h, w, g)
    assert 2 * 19 >= 38 and (328 // 8) * (280 // 8) == 1435
    print("oracle corners (alone, with existing):", counts)


# ---------------------------------------------------------------------------------------- pipeline
@pytest.mark.parametrize("case", R.PIPELINE_CASES, ids=lambda c: "%dx%d-L%d-g%d" % c[:4])
def test_pipeline_conditions(oracle, case):
    """On every frame the oracle keeps at least half of the previous frame's ids, and over the
    frames it loses at least one; the many-cell case passes 1024 list entries."""
    h, w, L, g, noise, k = case
    ref = oracle.StereoTracker(w, h, L, g, 20, 0.01)
    prev, lost, sizes = None, 0, []
    for i, (left, right) in enumerate(R.pipeline_frames(*case)):
        if i == 3:
            drop = np.array(prev[::3], np.uint64)
            ref.remove_ids(drop)
            prev = [x for x in prev if x not in set(drop.tolist())]
        rl, rr = ref.process_frame(left, right)
        ids = [f[0] for f in rl]
        sizes.append((len(rl), len(rr)))
        if prev is not None:
            kept = len(set(ids) & set(prev))
            assert 2 * kept >= len(prev), (i, kept, len(prev))
            lost += len(prev) - kept
        prev = ids
    assert lost >= 1
    if (h, w, L, g) == R.MANY_CELLS:
        assert min(sizes[2]) > 1024   # what frame 4 tracks from, and what remove_ids compacts
    print("oracle features per frame (left, right):", sizes, "lost:", lost)
