"""The motion covariance on the GPU (rsvio_motion_covariance*, rsvio_pnp_batch_covariance;
pnp_covariance.hpp) against tests/motion_covariance_reference.py: parity on well-conditioned frames
at a minimum and away from one, the statuses, the masks, the join's edges, the identities between
the entry points (bit for bit) and the Estimator option."""
import ctypes as C

import numpy as np
import pytest

import motion_covariance_reference as R
from oracle.pnp_reference import TOP_ID, build_table, map_bucket

pytestmark = pytest.mark.gpu


def _lists(m):
    return m.ids_l, m.uv_l, m.ids_r, m.uv_r


def _map(m):
    return m.map_ids, m.map_pw


def _frame(**kw):
    from rsvio import synthetic as S
    return S.motion_frame(**kw)


def _cov(mt, m, T, delta=2.0, masks=(None, None)):
    return mt.covariance(*_lists(m), T, m.T_C_B2, delta, *masks)


def _f64(x):
    return np.float64(x).tobytes()


def _bits(c):
    """Everything of a PoseCovariance but its timing, NaNs included."""
    return (c.status, c.cov.tobytes(), c.n_observations, c.n_downweighted, _f64(c.cost), _f64(c.min_pivot))


def _symmetric(c):
    return c.cov.tobytes() == np.ascontiguousarray(c.cov.T).tobytes()


def _all_nan(c):
    return c.cov.shape == (6, 6) and bool(np.isnan(c.cov).all())


@pytest.fixture(scope="module")
def mt(gpu):
    from rsvio.motion import MotionTracker
    t = MotionTracker()
    yield t
    t.close()


# ---------------------------------------------------------------- parity

PARITY = [(n, d) for n in R.PARITY_FRAMES for d in R.PARITY_DELTAS[n]]


@pytest.mark.parametrize("name,delta", PARITY)
def test_parity_with_the_reference(mt, name, delta):
    """Sigma within 1e-8 (scaled) of the reference, the counts exact, the cost within 1e-9, at the
    pose track_motion returns and at T_W_B_last_kf, which is no minimum.  The frame is re-seeded
    until no factor lies within 1e-9 (relative) of the Huber knee at either pose, so the count of
    down-weighted factors does not hang on rounding."""
    from rsvio.motion import pnp_cfg
    for seed in range(3, 9):
        m = _frame(seed=seed, **R.PARITY_FRAMES[name])
        mt.set_map(*_map(m))
        r = mt.track_motion(*_lists(m), m.T_W_B_last_kf, m.T_C_B2, cfg=pnp_cfg(huber_delta=delta))
        assert r.success
        poses = {"tracked": r.T_W_B, "last_kf": m.T_W_B_last_kf}
        margins = [R.knee_margin(_lists(m), _map(m), T, m.T_C_B2, delta) for T in poses.values()]
        if min(margins) > R.KNEE_MARGIN:
            break
    else:
        raise AssertionError("no seed keeps every factor off the Huber knee")
    for where, T in poses.items():
        H, S, cost, n, n_down = R.reference(_lists(m), _map(m), T, m.T_C_B2, delta)
        assert np.linalg.cond(H) <= R.KAPPA_MAX
        c = _cov(mt, m, T, delta)
        err = R.scaled_error(c.cov, S)
        rel_cost = abs(c.cost - cost) / cost
        print(f"{name} delta {delta} seed {seed} {where}: n {n} down {n_down} scaled error {err:.3e} "
              f"cost rel {rel_cost:.3e} min_pivot {c.min_pivot:.4g} kernel_ms {c.kernel_ms:.4f}")
        assert c.status == R.MCOV_OK
        assert (c.n_observations, c.n_downweighted) == (n, n_down)
        assert n == r.n_observations
        assert err <= R.PARITY_CAP
        assert rel_cost <= 1e-9
        assert _symmetric(c)
        assert c.min_pivot > 0 and c.kernel_ms > 0
        if where == "tracked":
            assert abs(c.cost - r.final_cost) <= 1e-9 * r.final_cost
    if delta < 1.0:
        assert n_down > 0            # the weights are active
    if name == "capacity":
        assert len(m.ids_l) + len(m.ids_r) == 4096


@pytest.mark.parametrize("masked", [True, False])
def test_three_factor_frame(mt, masked):
    """kappa is about 2e6 here, so parity is not asked: eps kappa 6 is about 2.4e-9, and the
    residual cap 1e-6 leaves more than two orders above it."""
    m = _frame(n_feat=3, unmapped=0)
    mt.set_map(*_map(m))
    masks = (np.ones(3, np.uint8), np.zeros(3, np.uint8)) if masked else (None, None)
    H, _, _, n, _ = R.reference(_lists(m), _map(m), m.T_W_B_true, m.T_C_B2, 2.0, masks if masked else None)
    c = _cov(mt, m, m.T_W_B_true, 2.0, masks)
    assert n == (3 if masked else 6) and c.n_observations == n
    assert c.status == R.MCOV_OK and _symmetric(c)
    res = float(np.abs(c.cov @ H - np.eye(6)).max())
    print(f"{n} factors: residual {res:.3e} min_pivot {c.min_pivot:.4g}")
    assert res <= 1e-6


# ---------------------------------------------------------------- statuses

def test_too_few(gpu, mt):
    from rsvio.motion import MotionTracker
    m = _frame(n_feat=20)
    none = (np.zeros(0, np.uint64), np.zeros((0, 2), np.float32))
    cases = {}
    mt.set_map(np.zeros(0, np.uint64), np.zeros((0, 3), np.float32))
    cases["an empty map"] = (_cov(mt, m, m.T_W_B_true), 0)
    fresh = MotionTracker()
    try:
        cases["no map set"] = (_cov(fresh, m, m.T_W_B_true), 0)
    finally:
        fresh.close()
    mt.set_map(*_map(m))
    cases["both lists empty"] = (mt.covariance(*none, *none, m.T_W_B_true, m.T_C_B2), 0)
    zeros = (np.zeros(len(m.ids_l), np.uint8), np.zeros(len(m.ids_r), np.uint8))
    cases["a mask of zeros"] = (_cov(mt, m, m.T_W_B_true, 2.0, zeros), 0)
    two = _frame(n_feat=1, unmapped=5)
    mt.set_map(*_map(two))
    cases["2 factors"] = (_cov(mt, two, two.T_W_B_true), 2)
    for what, (c, n) in cases.items():
        assert c.status == R.MCOV_TOO_FEW, what
        assert c.n_observations == n, what
        assert _all_nan(c), what
        assert c.min_pivot == 0.0, what
    assert cases["an empty map"][0].cost == 0.0
    _, _, cost, n, _ = R.reference(_lists(two), _map(two), two.T_W_B_true, two.T_C_B2, 2.0)
    assert n == 2 and abs(cases["2 factors"][0].cost - cost) <= 1e-9 * cost


def test_singular(mt):
    m = _frame(n_feat=20)
    mt.set_map(*_map(m))
    T = m.T_W_B_true.copy()
    T[1, 3] = np.nan
    c = _cov(mt, m, T)
    assert c.status == R.MCOV_SINGULAR and _all_nan(c) and c.n_observations == 40
    # a map point on the cameras' z = 0 plane among 4 factors: 1 / z is not finite, nor is H
    ids = np.array([1, 2, 3, 4], np.uint64)
    pw = np.array([[0, 0, 0], [1, 0, 4], [0, 1, 5], [1, 1, 6]], np.float32)
    mt.set_map(ids, pw)
    uv = (pw[:, :2] / np.maximum(pw[:, 2:3], 1)).astype(np.float32)
    eye2 = np.stack([np.eye(4).reshape(16)] * 2)
    c = mt.covariance(ids, uv, np.zeros(0, np.uint64), np.zeros((0, 2), np.float32), np.eye(4), eye2)
    assert c.status == R.MCOV_SINGULAR and _all_nan(c) and c.n_observations == 4
    # the same frame without that point is fine
    c = mt.covariance(ids[1:], uv[1:], np.zeros(0, np.uint64), np.zeros((0, 2), np.float32), np.eye(4), eye2)
    assert c.n_observations == 3 and c.status in (R.MCOV_OK, R.MCOV_SINGULAR)


# ---------------------------------------------------------------- masks

def test_masks(mt):
    m = _frame(n_feat=90, outlier_frac=0.2, seed=5)
    mt.set_map(*_map(m))
    rng = np.random.default_rng(11)
    half = tuple((rng.uniform(size=len(i)) < 0.5).astype(np.uint8) for i in (m.ids_l, m.ids_r))
    T, delta = m.T_W_B_true, 0.002
    assert R.knee_margin(_lists(m), _map(m), T, m.T_C_B2, delta, half) > R.KNEE_MARGIN
    H, S, cost, n, n_down = R.reference(_lists(m), _map(m), T, m.T_C_B2, delta, half)
    c = _cov(mt, m, T, delta, half)
    assert c.status == R.MCOV_OK and (c.n_observations, c.n_downweighted) == (n, n_down)
    assert 0 < n < 180 and n_down > 0
    assert np.linalg.cond(H) <= R.KAPPA_MAX and R.scaled_error(c.cov, S) <= R.PARITY_CAP
    assert abs(c.cost - cost) <= 1e-9 * cost
    # a 1 on a feature without a map point changes nothing; a 2 (the robust call's outlier) is not a 1
    mapped = tuple(np.isin(i, m.map_ids) for i in (m.ids_l, m.ids_r))
    assert not mapped[0].all() and not mapped[1].all()
    on_mapped = tuple((h & k).astype(np.uint8) for h, k in zip(half, mapped))
    plus_unmapped = tuple((h | ~k).astype(np.uint8) for h, k in zip(on_mapped, mapped))
    assert _bits(_cov(mt, m, T, delta, on_mapped)) == _bits(_cov(mt, m, T, delta, plus_unmapped)) == _bits(c)
    twos = tuple(np.where(h == 1, 1, 2).astype(np.uint8) for h in half)
    assert _bits(_cov(mt, m, T, delta, twos)) == _bits(c)
    # one list masked, the other not
    c_l = _cov(mt, m, T, delta, (half[0], None))
    n_l = R.reference(_lists(m), _map(m), T, m.T_C_B2, delta, (half[0], None))[3]
    assert c_l.n_observations == n_l > n


def test_masks_of_the_robust_call(mt):
    import robust_motion_reference as RR
    from rsvio.motion import RansacConfig
    m, uv_l, uv_r, _, _ = RR.corrupted_frame()
    mt.set_map(*_map(m))
    r = mt.track_motion_robust(m.ids_l, uv_l, m.ids_r, uv_r, m.T_W_B_last_kf, m.T_C_B2, RansacConfig(n_hyp=64, seed=1))
    assert r.motion.success and 3 <= r.n_inliers < int((r.mask_l != 0).sum() + (r.mask_r != 0).sum())
    c = mt.covariance(m.ids_l, uv_l, m.ids_r, uv_r, r.motion.T_W_B, m.T_C_B2, 2.0, r.mask_l, r.mask_r)
    assert c.status == R.MCOV_OK and c.n_observations == r.n_inliers
    assert _symmetric(c) and np.all(np.diag(c.cov) > 0)


# ---------------------------------------------------------------- the join's edges

def _renamed(m, new_map_ids):
    """m with its map ids replaced by new_map_ids (ascending: rank for rank), features re-sorted."""
    import dataclasses
    new_map_ids = np.asarray(new_map_ids, np.uint64)
    assert len(new_map_ids) == len(m.map_ids) and np.all(new_map_ids[1:] > new_map_ids[:-1])
    out = {}
    for s in ("l", "r"):
        ids, uv = getattr(m, "ids_" + s).copy(), getattr(m, "uv_" + s)
        ok = np.isin(ids, m.map_ids)
        ids[ok] = new_map_ids[np.searchsorted(m.map_ids, ids[ok])]
        assert not np.isin(ids[~ok], new_map_ids).any()
        order = np.argsort(ids, kind="stable")
        out["ids_" + s], out["uv_" + s] = ids[order], uv[order]
    return dataclasses.replace(m, map_ids=new_map_ids, **out)


def _edge_parity(mt, m):
    mt.set_map(*_map(m))
    H, S, cost, n, n_down = R.reference(_lists(m), _map(m), m.T_W_B_true, m.T_C_B2, 2.0)
    c = _cov(mt, m, m.T_W_B_true)
    assert c.status == R.MCOV_OK and (c.n_observations, c.n_downweighted) == (n, n_down)
    assert np.linalg.cond(H) <= R.KAPPA_MAX and R.scaled_error(c.cov, S) <= R.PARITY_CAP
    assert abs(c.cost - cost) <= 1e-9 * cost
    return n


def test_ids_chained_past_the_first_bucket(mt):
    m = _frame(n_map=12, n_feat=12, unmapped=3)
    chain = [i for i in range(1, 4000) if map_bucket(i, 15) == 3][:12]     # 12 ids, one home bucket of 4
    table = build_table(chain)
    assert table["buckets"] == 16 and table["max_probe"] == 2
    m = _renamed(m, chain)
    assert _edge_parity(mt, m) == 24
    assert mt.map_stats()["max_probe"] == 2


def test_the_top_id(mt):
    m = _frame(n_map=12, n_feat=12, unmapped=3)
    ids = m.map_ids.copy()
    ids[-1] = np.uint64(TOP_ID)
    m = _renamed(m, ids)
    assert m.ids_l[-1] == np.uint64(TOP_ID) and m.ids_r[-1] == np.uint64(TOP_ID)
    assert _edge_parity(mt, m) == 24
    assert mt.map_stats()["has_top"] == 1


# ---------------------------------------------------------------- path identities

def test_two_calls_give_the_same_bits(mt):
    m = _frame(outlier_frac=0.3)
    mt.set_map(*_map(m))
    a, b = (_cov(mt, m, m.T_W_B_last_kf, 0.002) for _ in range(2))
    assert a.status == R.MCOV_OK and _bits(a) == _bits(b)


def test_track_motion_after_a_covariance_call(gpu):
    """The call leaves no state behind: track_motion on the handle equals one on a fresh handle."""
    from rsvio.motion import MotionTracker
    m = _frame()
    other = _frame(n_feat=50, seed=9)
    res = []
    for with_cov in (True, False):
        t = MotionTracker()
        try:
            t.set_map(*_map(m))
            if with_cov:
                mask = (np.arange(len(other.ids_l)) % 2).astype(np.uint8)
                # another frame's lists, a mask and another delta through the handle's staging first
                # (its ids are drawn from the same range: a few of them are in this map)
                assert _cov(t, other, other.T_W_B_true, 0.5, (mask, None)).n_observations < len(other.ids_l)
                assert _cov(t, m, m.T_W_B_true).status == R.MCOV_OK
            r = t.track_motion(*_lists(m), m.T_W_B_last_kf, m.T_C_B2)
            res.append((r.status, r.iterations, r.is_keyframe, r.n_observations, _f64(r.initial_cost),
                        _f64(r.final_cost), _f64(r.translation_norm), _f64(r.rotation_norm), r.T_W_B.tobytes()))
        finally:
            t.close()
    assert res[0] == res[1] and res[0][0] > 0


def test_tracker_fed_call_equals_the_host_lists(gpu):
    from rsvio import synthetic as S
    from rsvio.camera import EUROC
    from rsvio.motion import MotionTracker
    w, h = 320, 240
    tex = S.make_texture(w, h, n_blobs=1600, seed=99)
    rng = np.random.default_rng(100)
    frames = [(S._render(tex, w, h, t, False, 2 * rng.standard_normal((h, w))),
               S._render(tex, w, h, t, True, 2 * rng.standard_normal((h, w)))) for t in range(2)]
    trk = gpu.StereoPatchTracker(w, h, levels=3, grid_size=30)
    trk.set_cameras(*EUROC)
    t = MotionTracker()
    try:
        trk.process_frame(*frames[0])
        fl, fr = trk.process_frame(*frames[1])
        ul, ur = trk.undistorted()
        T_C_B2 = np.stack([np.linalg.inv(S.T_B_CL).reshape(16), np.linalg.inv(S.T_B_CR).reshape(16)])
        ids = fl["id"].astype(np.uint64)
        rays = np.concatenate([ul.astype(np.float64), np.ones((len(ul), 1))], 1) * 4.0
        p_W = (S.T_B_CL[:3, :3] @ rays.T).T + S.T_B_CL[:3, 3]
        keep = np.arange(len(ids)) % 3 != 0          # a third of the tracks are not in the map
        t.set_map(ids[keep], p_W[keep].astype(np.float32))
        T = np.eye(4)
        T[:3, 3] = [0.01, -0.02, 0.005]
        mask_l = (np.arange(len(fl)) % 4 != 1).astype(np.uint8)
        mask_r = (np.arange(len(fr)) % 5 != 2).astype(np.uint8)
        for masks in ((None, None), (mask_l, mask_r), (mask_l, None)):
            d = t.covariance_tracker(trk, T, T_C_B2, 2.0, *masks)
            s = t.covariance(ids, ul, fr["id"].astype(np.uint64), ur, T, T_C_B2, 2.0, *masks)
            assert _bits(d) == _bits(s)
            assert d.n_observations >= 3 and d.status in (R.MCOV_OK, R.MCOV_SINGULAR)
        print(f"tracker-fed: {len(fl)} + {len(fr)} features, {d.n_observations} factors, status {d.status}")
        assert t.covariance_tracker(trk, T, T_C_B2).n_observations > 10
    finally:
        t.close()
        trk.close()


def _combos():
    """(frame, masks) per handle: ragged sizes, one with active weights."""
    out = []
    for kw in (dict(n_feat=8, seed=1), dict(n_feat=65, seed=2), dict(n_feat=300, seed=3),
               dict(n_feat=40, outlier_frac=0.3, seed=4)):
        out.append(_frame(n_map=400, **kw))
    return out


def _slot(i, combos):
    """Slot i of a batch: (handle index, lists, T_W_B, masks); slot 1 is an empty frame, every fifth
    slot from 2 is masked, the poses alternate between the true one and the last keyframe's."""
    k = i % len(combos)
    m = combos[k]
    lists = _lists(m)
    masks = None
    if i == 1:
        lists = (np.zeros(0, np.uint64), np.zeros((0, 2), np.float32)) * 2
    elif i % 5 == 2:
        rng = np.random.default_rng(i)
        masks = ((rng.uniform(size=len(m.ids_l)) < 0.6).astype(np.uint8), None if i % 2 else
                 (rng.uniform(size=len(m.ids_r)) < 0.6).astype(np.uint8))
    return k, lists, (m.T_W_B_true if i % 2 else m.T_W_B_last_kf), masks


@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("on_device", [False, True])
def test_batch_equals_the_single_calls(gpu, n, on_device):
    import torch

    from rsvio.motion import MotionBatch, MotionFrame, MotionTracker
    combos = _combos()
    mts = [MotionTracker() for _ in combos]
    mb = None
    try:
        for t, m in zip(mts, combos):
            t.set_map(*_map(m))
        slots = [_slot(i, combos) for i in range(n)]
        delta = 0.002
        single = [mts[k].covariance(*lists, T, combos[k].T_C_B2, delta, *(masks or (None, None)))
                  for k, lists, T, masks in slots]
        frames, keep = [], []
        for i, (k, lists, T, masks) in enumerate(slots):
            if on_device and i % 3 != 1:      # ids 24 bytes apart in a device buffer, uv as device tensors
                dev = []
                for ids, uv in (lists[:2], lists[2:]):
                    buf = np.full((len(ids), 24), 0xEE, np.uint8)
                    buf[:, :8] = np.ascontiguousarray(ids, np.uint64).view(np.uint8).reshape(-1, 8)
                    dev += [torch.from_numpy(buf.reshape(-1)).cuda(),
                            torch.from_numpy(np.ascontiguousarray(uv, np.float32)).cuda()]
                keep.append(dev)
                frames.append(MotionFrame(*dev, None, combos[k].T_C_B2, on_device=True, id_stride=24))
            else:
                frames.append(MotionFrame(*lists, None, combos[k].T_C_B2))
        torch.cuda.synchronize()
        mb = MotionBatch([mts[k] for k, *_ in slots])
        got = mb.covariance(frames, np.stack([T for _, _, T, _ in slots]), delta, [s[3] for s in slots])
        again = mb.covariance(frames, np.stack([T for _, _, T, _ in slots]), delta, [s[3] for s in slots])
        assert len(got) == n and mb.device_ms > 0
        for i, (g, a, s) in enumerate(zip(got, again, single)):
            assert _bits(g) == _bits(s), i
            assert _bits(a) == _bits(s), i
        assert got[0].status == R.MCOV_OK and got[0].n_observations == 16
        if n > 1:
            assert got[1].status == R.MCOV_TOO_FEW and got[1].n_observations == 0 and _all_nan(got[1])
        if n > 2:
            assert got[2].status == R.MCOV_OK and 3 <= got[2].n_observations < 600
            assert sum(g.n_downweighted for g in got) > 0
    finally:
        if mb is not None:
            mb.close()
        for t in mts:
            t.close()


# ---------------------------------------------------------------- refusals

def test_refusals(gpu, mt):
    from rsvio import RsvioError
    from rsvio.motion import MotionBatch, MotionFrame
    m = _frame(n_feat=20)
    mt.set_map(*_map(m))
    ids = np.arange(4097, dtype=np.uint64)
    uv = np.zeros((4097, 2), np.float32)
    none = (np.zeros(0, np.uint64), np.zeros((0, 2), np.float32))
    with pytest.raises(RsvioError) as e:
        mt.covariance(ids, uv, *none, m.T_W_B_true, m.T_C_B2)
    assert e.value.code == -4
    with pytest.raises(RsvioError) as e:
        mt.covariance(ids[:2049], uv[:2049], ids[:2048], uv[:2048], m.T_W_B_true, m.T_C_B2)
    assert e.value.code == -4
    for delta in (0.0, -2.0, float("nan")):
        with pytest.raises(RsvioError) as e:
            _cov(mt, m, m.T_W_B_true, delta)
        assert e.value.code == -1
    mb = MotionBatch([mt, mt, mt])
    try:
        ok = MotionFrame(*_lists(m), None, m.T_C_B2)
        big = MotionFrame(ids, uv, *none, None, m.T_C_B2)
        T = np.stack([m.T_W_B_true] * 3)
        with pytest.raises(RsvioError) as e:
            mb.covariance([ok, big, ok], T)
        assert e.value.code == -4 and "slot 1" in str(e.value)
        with pytest.raises(RsvioError) as e:
            mb.covariance([ok, ok, ok], T, 0.0)
        assert e.value.code == -1
        assert [c.status for c in mb.covariance([ok, ok, ok], T)] == [R.MCOV_OK] * 3
    finally:
        mb.close()
    from rsvio import _lib
    assert C.sizeof(_lib.MotionCovInfo) == 40


# ---------------------------------------------------------------- Estimator

def test_estimator_pose_covariance(gpu):
    """12 frames at 376 x 240, window 5: with pose_covariance on, every field a FrameResult has today
    equals the run with it off; the covariance is there exactly on the frames whose motion tracking
    succeeded and equals MotionTracker.covariance on the collected lists at the frame's T_W_B."""
    import dataclasses

    from rsvio import synthetic as S
    from rsvio.camera import Camera
    from rsvio.estimator import DeviceBackend, Estimator
    from rsvio.motion import MotionTracker
    s = S.euroc_scene_stream(12, w=376, h=240)
    h, w = s.frames[0][0].shape
    cams = [Camera.opencv5(*p) for p in s.intrinsics]
    calls = []

    class Recording(DeviceBackend):
        def collect(self):
            self.feats = super().collect()
            return self.feats

        def set_map(self, ids, p_W):
            self.map = (np.array(ids, np.uint64), np.array(p_W, np.float32))
            super().set_map(ids, p_W)

        def pose_covariance(self, T_W_B, T_C_B2, huber_delta, mask_l=None, mask_r=None):
            assert mask_l is None and mask_r is None
            c = super().pose_covariance(T_W_B, T_C_B2, huber_delta, mask_l, mask_r)
            calls.append((self.feats, self.map, np.array(T_W_B), np.array(T_C_B2), huber_delta, c))
            return c

    runs = []
    for on in (False, True):
        be = Recording(w, h, cams, 4, 25, 20, 0.01, 5, 0.05, 0.05, 0)
        est = Estimator(w, h, cams, s.T_B_Cl, s.T_B_Cr, window=5, backend=be, pose_covariance=on)
        runs.append(list(est.run(s.frames)))
        est.close()
        if not on:
            assert calls == []
    off, on = runs
    assert len(off) == len(on) == 12
    today = [f.name for f in dataclasses.fields(off[0]) if f.name != "pose_covariance"]
    tracked = 0
    for x, y in zip(off, on):
        for name in today:
            a, b = getattr(x, name), getattr(y, name)
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, name
        assert x.pose_covariance is None
        if y.pnp_status is not None and y.pnp_status > 0:
            tracked += 1
            P = y.pose_covariance
            assert P.shape == (6, 6) and np.isfinite(P).all() and np.array_equal(P, P.T)
            assert np.all(np.diag(P) > 0)
        else:
            assert y.pose_covariance is None
    assert tracked >= 3 and len(calls) == tracked
    mt = MotionTracker()
    try:
        it = iter(calls)
        for y in on:
            if y.pose_covariance is None:
                continue
            ((ids_l, uv_l), (ids_r, uv_r)), map_, T, tcb, delta, c = next(it)
            assert delta == 2.0 and c.status == R.MCOV_OK
            mt.set_map(*map_)
            ref = mt.covariance(ids_l.astype(np.uint64), uv_l, ids_r.astype(np.uint64), uv_r, T, tcb, delta)
            assert _bits(ref) == _bits(c)
            assert ref.cov.tobytes() == y.pose_covariance.tobytes()
            assert abs(c.cost - y.pnp_cost) <= 1e-9 * y.pnp_cost
    finally:
        mt.close()
