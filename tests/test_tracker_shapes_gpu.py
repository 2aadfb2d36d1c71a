"""GPU parity of the patch tracker at every pyramid depth, on ragged shapes and at the edges of the
LK parameters, bit for bit against the CPU oracle (seeded tracking: tests/seeded_tracking_reference.py).

What each shape is for, and that it still serves it, is checked without a device in
test_tracker_shapes_cpu.py; the inputs and case tables are tests/tracker_shapes_reference.py's.
The pyramid tests read PyramidPlan::init's decisions back (rsvio_dbg_pyramid_plan), so a shape that
no longer takes the path it was chosen for fails instead of passing on another path.
"""
import ctypes as C

import numpy as np
import pytest

import tracker_shapes_reference as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _plan(w, h, levels):
    """rsvio_dbg_pyramid_plan: (tile_w[8], tile_h[8], direct, lds_bytes)"""
    from rsvio import _lib
    tw, th = np.full(8, -1, np.int32), np.full(8, -1, np.int32)
    direct, lds = C.c_uint32(0xFFFFFFFF), C.c_uint64(0)
    _lib.check(_lib.load().rsvio_dbg_pyramid_plan(w, h, levels, _lib.ptr(tw), _lib.ptr(th), C.byref(direct),
                                                  C.byref(lds)))
    return tw.tolist(), th.tolist(), direct.value, lds.value


# ----------------------------------------------------------------------------------------- pyramid
@pytest.mark.parametrize("case", R.PYRAMID_CASES, ids=lambda c: "%dx%d-L%d" % c[:3])
def test_pyramid_host_bitexact(gpu, oracle, case):
    h, w, L, direct = case
    tw, th, got_direct, lds = _plan(w, h, L)
    ref = R.pyramid_plan(w, h, L)
    assert (tw, th, got_direct, lds) == (ref["tile_w"], ref["tile_h"], ref["direct"], ref["lds_bytes"])
    assert lds <= 65536
    if direct is not None:
        assert got_direct == direct
    images = [R.noise_image(h, w, L)]
    if (h, w) in R.DIRECT_SHAPES:
        images.append(R.texture(h, w, 3))   # noise alone rounds level 7 to 127 / 128
    for img in images:
        want = oracle.build_pyramid(img, L)
        out = gpu.build_image_pyramid(img, L)
        assert out.shape == want.shape
        assert np.array_equal(out, want)


def test_pyramid_plan_rejects_bad_arguments(gpu):
    from rsvio import _lib
    lib = _lib.load()
    tw, th = np.zeros(8, np.int32), np.zeros(8, np.int32)
    d, n = C.c_uint32(0), C.c_uint64(0)
    assert lib.rsvio_dbg_pyramid_plan(64, 64, 9, _lib.ptr(tw), _lib.ptr(th), C.byref(d), C.byref(n)) < 0
    assert lib.rsvio_dbg_pyramid_plan(64, 64, 3, None, _lib.ptr(th), C.byref(d), C.byref(n)) < 0


def _packed_pyramids(oracle, imgs, L, src_off=0, dst_off=0):
    """rsvio_build_pyramids_d on packed images inside larger device buffers, the images' base src_off
    bytes and the pyramids' base dst_off bytes past a 64-byte boundary; every pyramid against the
    oracle, and every byte around them still the 0xA5 fill."""
    import torch

    from rsvio import _lib
    lib = _lib.load()
    n, h, w = imgs.shape
    dev = torch.device("cuda", 0)
    pb = int(lib.rsvio_pyramid_bytes(w, h, L))
    guard = 64
    d_src = torch.zeros(guard + src_off + n * h * w, dtype=torch.uint8, device=dev)
    d_src[guard + src_off:] = torch.from_numpy(imgs.reshape(-1)).to(dev)
    d_dst = torch.full((guard + dst_off + n * pb + guard,), 0xA5, dtype=torch.uint8, device=dev)
    assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
    ctx = C.c_void_p()
    _lib.check(lib.rsvio_track_ctx_create(w, h, L, 0, C.byref(ctx)))
    try:
        _lib.check(lib.rsvio_build_pyramids_d(ctx, d_src.data_ptr() + guard + src_off, n,
                                              d_dst.data_ptr() + guard + dst_off, None))
        torch.cuda.synchronize()
    finally:
        lib.rsvio_track_ctx_destroy(ctx)
    out = d_dst.cpu().numpy()
    lo = guard + dst_off
    assert np.all(out[:lo] == 0xA5) and np.all(out[lo + n * pb:] == 0xA5)
    for i in range(n):
        assert np.array_equal(out[lo + i * pb:lo + (i + 1) * pb], oracle.build_pyramid(imgs[i], L)), i


@pytest.mark.parametrize("case", R.PACKED_CASES, ids=lambda c: "%dx%dx%d-L%d" % c)
def test_pyramids_packed_unaligned(gpu, oracle, case):
    """w * h % 16 != 0: image 1 onward has an unaligned source and destination (byte-wise level-0
    copy and byte strip staging) while image 0 of the same launch takes the 16-byte path."""
    n, h, w, L = case
    imgs = np.stack([R.noise_image(h, w, L, k) for k in range(n)])
    _packed_pyramids(oracle, imgs, L)


@pytest.mark.parametrize("src_off,dst_off", [(4, 0), (0, 1)])
def test_pyramids_packed_offset_base(gpu, oracle, src_off, dst_off):
    """w % 4 == 0 and an aligned image size, but a base off the 16-byte boundary: the unaligned
    branch on every image, by the source alone and by the destination alone."""
    n, h, w, L = R.OFFSET_CASE
    assert (h * w) % 16 == 0 and w % 4 == 0
    imgs = np.stack([R.noise_image(h, w, L, k) for k in range(n)])
    _packed_pyramids(oracle, imgs, L, src_off, dst_off)


# ---------------------------------------------------------------------------------------------- LK
@pytest.fixture(scope="module")
def depth(oracle):
    h, w = R.DEPTH_SHAPE
    a, b = R.shifted_pair(h, w, 11)
    return oracle.build_pyramid(a, 8), oracle.build_pyramid(b, 8), R.lk_states(h, w, 96, 5)


@pytest.mark.parametrize("L", range(1, 9))
def test_lk_every_depth(gpu, oracle, depth, L):
    """make_templates<L> for every L (one part, a full first part, a second part of 1 .. 4 levels)."""
    h, w = R.DEPTH_SHAPE
    p0, p1, aff = depth
    nb = oracle.pyramid_bytes(w, h, L)
    ra, rv = oracle.track_points(p0[:nb], p1[:nb], w, h, L, aff)
    ga, gv = gpu.track_points(p0[:nb], p1[:nb], w, h, L, aff)
    assert np.array_equal(gv, rv)
    assert np.array_equal(_bits(ga), _bits(ra))


@pytest.mark.parametrize("L", range(1, 9))
def test_lk_every_depth_seeded(gpu, depth, L):
    """The same through rsvio_track_points_seeded: a third of the seeds exact, a third 1.5 px off,
    a third NaN (the own position)."""
    import seeded_tracking_reference as SR
    from oracle import oracle as O
    h, w = R.DEPTH_SHAPE
    p0, p1, aff = depth
    nb = O.pyramid_bytes(w, h, L)
    seeds = R.lk_seeds(aff, R.DEPTH_SHIFT)
    ra, rv = SR.track_points_seeded(p0[:nb], p1[:nb], w, h, L, aff, seeds)
    ga, gv = gpu.track_points_seeded(p0[:nb], p1[:nb], w, h, L, aff, seeds)
    assert np.array_equal(gv, rv)
    assert np.array_equal(_bits(ga), _bits(ra))
    assert rv.sum() >= 24


@pytest.mark.parametrize("case", R.UNDERSIZED_CASES + [R.MIXED_CASE], ids=lambda c: "%dx%d-L%d" % c)
def test_lk_undersized_top_levels(gpu, oracle, case):
    """Top levels of 1 x 1 (where `width - 2` wraps) and 3 x 3 (under 5 x 5: not sampled at all) and
    of 5 x 6: every state rejected and handed back unchanged; the mixed companion keeps some."""
    h, w, L = case
    a, b = R.shifted_pair(h, w, 20 + L)
    p0, p1 = oracle.build_pyramid(a, L), oracle.build_pyramid(b, L)
    aff = R.lk_states(h, w, 64, 6)
    ra, rv = oracle.track_points(p0, p1, w, h, L, aff)
    ga, gv = gpu.track_points(p0, p1, w, h, L, aff)
    assert np.array_equal(gv, rv)
    assert np.array_equal(_bits(ga), _bits(ra))
    if case != R.MIXED_CASE:
        assert not gv.any()
        assert np.array_equal(_bits(ga), _bits(aff))
    else:
        assert gv.any() and not gv.all()


@pytest.fixture(scope="module")
def edge(oracle):
    h, w, L = R.EDGE_SHAPE
    a, b = R.edge_pair()
    return oracle.build_pyramid(a, L), oracle.build_pyramid(b, L), R.lk_states(h, w, 96, 8)


@pytest.mark.parametrize("max_it,thresh", R.EDGE_COMBOS, ids=lambda v: repr(v))
def test_lk_parameter_edges(gpu, oracle, edge, max_it, thresh):
    """Both forms of the convergence test (a normal finite thresh: the midpoint square; zero,
    subnormal, infinite, NaN, negative: the square root) and max_iterations 0, 1, 2 (the last
    update's out-of-bound flag consumed after the loop)."""
    h, w, L = R.EDGE_SHAPE
    p0, p1, aff = edge
    ra, rv = oracle.track_points(p0, p1, w, h, L, aff, max_it, thresh)
    ga, gv = gpu.track_points(p0, p1, w, h, L, aff, max_it, thresh)
    assert np.array_equal(gv, rv)
    assert np.array_equal(_bits(ga), _bits(ra))


# -------------------------------------------------------------------------------------------- FAST
@pytest.mark.parametrize("case", R.FAST_CASES, ids=lambda c: "%dx%d-g%d" % c)
def test_fast_grid_geometry(gpu, oracle, case):
    """Grid extremes (w % g == 0, g = 8, g = 128, one cell, no candidate inside the border, more
    than 1024 cells), without existing points and with points on the bin edges."""
    h, w, g = case
    img = R.fast_image(h, w, g)
    ref = oracle.detect_key_points(img, g)
    out = gpu.detect_key_points(img, g)
    assert np.array_equal(out[0], ref[0]) and np.array_equal(_bits(out[1]), _bits(ref[1]))
    existing = R.fast_existing(h, w, g, ref[0])
    ref2 = oracle.detect_key_points(img, g, existing)
    out2 = gpu.detect_key_points(img, g, existing)
    assert np.array_equal(out2[0], ref2[0]) and np.array_equal(_bits(out2[1]), _bits(ref2[1]))
    assert len(ref2[0]) < len(ref[0]) or case == R.FAST_EMPTY


# ---------------------------------------------------------------------------------------- pipeline
def _same_lists(ref_lists, gpu_lists, what):
    """_pipeline_compare's comparison (test_tracker_gpu.py): ids, counts, positions and rotations."""
    for refl, gpul in zip(ref_lists, gpu_lists):
        assert len(refl) == len(gpul), what
        assert [f[0] for f in refl] == gpul["id"].tolist(), what
        assert np.array_equal(_bits(np.array([f[1] for f in refl], np.float32)), _bits(gpul["x"])), what
        assert np.array_equal(_bits(np.array([f[2] for f in refl], np.float32)), _bits(gpul["y"])), what
        assert np.array_equal(_bits(np.array([f[3][:4] for f in refl], np.float32).reshape(-1, 4)),
                              _bits(gpul["r"].reshape(-1, 4))), what


@pytest.mark.parametrize("case", R.PIPELINE_CASES, ids=lambda c: "%dx%d-L%d-g%d" % c[:4])
def test_pipeline_shapes(gpu, oracle, case):
    """StereoPatchTracker against the oracle frame by frame; the many-cell case (1435 cells, lists
    past 1024 entries: more than one item per thread in the frame end's single workgroups) also
    removes every third id after frame 3 and runs a fourth frame."""
    h, w, L, g, noise, k = case
    ref = oracle.StereoTracker(w, h, L, g, 20, 0.01)
    trk = gpu.StereoPatchTracker(w, h, levels=L, grid_size=g)
    try:
        for i, (left, right) in enumerate(R.pipeline_frames(*case)):
            if i == 3:
                assert len(gl) > 1024 and len(gr) > 1024
                drop = gl["id"][::3].copy()
                ref.remove_ids(drop)
                trk.remove_id(drop)
                kept = trk.get_track_points()[0]
                assert not set(drop.tolist()) & set(kept) and len(kept) == len(gl) - len(drop)
            rl, rr = ref.process_frame(left, right)
            gl, gr = trk.process_frame(left, right)
            _same_lists((rl, rr), (gl, gr), f"frame {i}")
    finally:
        trk.close()


def test_pipeline_batched_ragged(gpu):
    """Two handles of the odd-width shape through the batched entry give the single handles' lists
    byte for byte."""
    h, w, L, g = R.BATCH_CASE
    seqs = [R.shifted_frames(h, w, 3, 1000 + h + L, 16), R.shifted_frames(h, w, 3, 77, 8)]
    singles = [gpu.StereoPatchTracker(w, h, levels=L, grid_size=g) for _ in seqs]
    batched = [gpu.StereoPatchTracker(w, h, levels=L, grid_size=g) for _ in seqs]
    tb = gpu.TrackerBatch(batched)
    try:
        for k in range(3):
            res = tb.process_frames([s[k][0] for s in seqs], [s[k][1] for s in seqs])
            assert tb.status == [0, 0]
            for t, s, (bl, br) in zip(singles, seqs, res):
                sl, sr = t.process_frame(s[k][0], s[k][1])
                assert len(sl) > 0
                assert bl.tobytes() == sl.tobytes() and br.tobytes() == sr.tobytes(), k
    finally:
        tb.close()
        for t in singles + batched:
            t.close()
