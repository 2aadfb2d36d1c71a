"""Batched motion tracking on the GPU (rsvio_pnp_batch_*: MotionBatch): one frame per handle in one
launch (three on the robust path).  The reference of every assertion is the single-stream call
(MotionTracker.track_motion / track_motion_robust) on the same handle with the same map, and the
comparison is test_motion_edges_gpu._bits': every integer, T_W_B, both costs and both norms as
bytes; kernel_ms is only required to be positive.  Inputs: oracle/pnp_cases.py,
rsvio.synthetic.motion_frame and tests/robust_motion_reference.corrupted_frame."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import robust_motion_reference as R
from oracle import pnp_cases as PC
from test_motion_edges_gpu import _bits, _check, _oracle
from test_robust_motion_gpu import Scene, _points

pytestmark = pytest.mark.gpu

LM_POSE = [("lm", n) for n in PC.LM_CASES] + [("pose", n) for n in PC.POSE_CASES]


def _frame(c, cfg=True):
    """A catalogue case as a slot's frame, with its own cfg."""
    from rsvio.motion import MotionFrame, pnp_cfg
    return MotionFrame(c.ids_l, c.uv_l, c.ids_r, c.uv_r, c.T_last, c.T_C_B2, cfg=pnp_cfg(**c.cfg) if cfg else None)


def _single(mt, c):
    from rsvio.motion import pnp_cfg
    return mt.track_motion(c.ids_l, c.uv_l, c.ids_r, c.uv_r, c.T_last, c.T_C_B2, cfg=pnp_cfg(**c.cfg))


def _same(batch_results, single_results):
    assert len(batch_results) == len(single_results)
    for i, (b, s) in enumerate(zip(batch_results, single_results)):
        assert _bits(b) == _bits(s), f"slot {i}"
        assert b.kernel_ms > 0.0


class Handles:
    """MotionTrackers that close together."""

    def __init__(self, n):
        from rsvio.motion import MotionTracker
        self.mt = [MotionTracker() for _ in range(n)]

    def __enter__(self):
        return self.mt

    def __exit__(self, *exc):
        for m in self.mt:
            m.close()


def _count_slice(n_l, n_r):
    """COUNT_CASES' frame (2,140 + 2,140 features) cut to n_l + n_r."""
    full = PC.get("count", "n2140+1956")
    m = PC._frame(seed=5, n_map=2300, n_feat=2100)
    return dataclasses.replace(full, ids_l=m.ids_l[:n_l], uv_l=m.uv_l[:n_l], ids_r=m.ids_r[:n_r], uv_r=m.uv_r[:n_r])


# ---------------------------------------------------------------- 1. mixed exits in one batch

def test_mixed_exits_in_one_batch(gpu, oracle):
    """Every LM exit, rejected steps, non-finite input and one to three features side by side, each
    slot with its own cfg, handle and map."""
    from rsvio.motion import MotionBatch
    cases = [PC.get(g, n) for g, n in LM_POSE]
    with Handles(len(cases)) as mts:
        for mt, c in zip(mts, cases):
            mt.set_map(c.map_ids, c.map_pw)
        single = [_single(mt, c) for mt, c in zip(mts, cases)]
        for c, s in zip(cases, single):
            if c.expect is not None:
                assert (s.status, s.iterations) == c.expect, c.name
        seen = {(s.status, s.iterations) for s in single}
        assert {(3, 0), (1, 21), (-1, 1), (-3, 1)} <= seen   # 0 and 21 iterations, NUMFAIL, LINSOLVE
        mb = MotionBatch(mts)
        frames = [_frame(c) for c in cases]
        a = mb.track_motion(frames)
        assert mb.device_ms > 0.0
        _same(a, single)
        names = [n for _, n in LM_POSE]
        for name in ("clean", "big-rot-B30", "tiny-2"):   # ... and against the oracle, the 1e-9 contract
            i = names.index(name)
            _check(a[i], _oracle(oracle, cases[i]), f"batch {name}")
        b = mb.track_motion(frames)
        assert [_bits(x) for x in a] == [_bits(x) for x in b]
        mb.close()
        perm = np.random.default_rng(7).permutation(len(cases))
        mp = MotionBatch([mts[k] for k in perm])
        p = mp.track_motion([frames[k] for k in perm])
        assert [_bits(x) for x in p] == [_bits(a[k]) for k in perm]
        mp.close()


# ---------------------------------------------------------------- 2. empty and full slots

def test_empty_and_full_slots(gpu):
    from rsvio import RsvioError, _lib
    from rsvio.motion import MotionBatch, pnp_cfg
    full = PC.get("count", "n2048+2048")
    cases = [_count_slice(0, 0), PC.get("count", "n64+64"), PC.get("count", "n512+0"), PC.get("count", "n0+2140"),
             full, PC.get("count", "n1+1")]
    with Handles(2) as (mt, empty):
        mt.set_map(full.map_ids, full.map_pw)
        empty.set_map(full.map_ids[:0], full.map_pw[:0])
        hs = [mt, empty, mt, mt, mt, mt]
        single = [_single(h, c) for h, c in zip(hs, cases)]
        assert single[0].status == -2 and single[0].n_observations == 0 and single[0].is_keyframe
        assert single[1].status == -2 and single[1].n_observations == 0
        assert single[2].n_observations == cases[2].n_obs > 0 and single[3].n_observations == cases[3].n_obs > 0
        assert len(full.ids_l) + len(full.ids_r) == 4096 and single[4].n_observations == full.n_obs
        assert single[5].success
        mb = MotionBatch(hs)
        frames = [_frame(c) for c in cases]
        _same(mb.track_motion(frames), single)
        # 4,097 features in slot 3: refused on the host, the slot named, nothing written
        k = 3
        frames[k] = _frame(_count_slice(2140, 1957))
        with pytest.raises(RsvioError) as e:
            mb.track_motion(frames)
        assert e.value.code == -4 and f"slot {k}" in str(e.value)
        tab, keep = mb._frames(frames)
        res = (_lib.MotionResult * mb.n)()
        C.memset(C.addressof(res), 0xA5, C.sizeof(res))
        cfg = pnp_cfg()
        rc = _lib.load().rsvio_pnp_batch_track_motion(mb._h, C.addressof(tab), C.byref(cfg), C.byref(mb.rule),
                                                      C.addressof(res), None)
        assert rc == -4 and bytes(res) == b"\xa5" * C.sizeof(res)
        # no cfg at all for a frame: INVALID_ARG, nothing written
        tab[1].cfg = None
        tab[k].n_r = 1956
        rc = _lib.load().rsvio_pnp_batch_track_motion(mb._h, C.addressof(tab), None, C.byref(mb.rule),
                                                      C.addressof(res), None)
        assert rc == -1 and bytes(res) == b"\xa5" * C.sizeof(res)
        mb.close()


# ---------------------------------------------------------------- 3. the CAP edge

@pytest.mark.parametrize("n_l,n_r", [(512, 512), (513, 512)])
def test_largest_frame_at_the_cap_edge(gpu, n_l, n_r):
    """1,024 features in the largest frame: the kernels with LDS for 1,024; 1,025: for 4,096."""
    from rsvio.motion import MotionBatch
    cases = [PC.get("count", f"n{n_l}+{n_r}"), PC.get("count", "n1+1"), PC.get("count", "n63+1"),
             PC.get("count", "n256+257")]
    assert len(cases[0].ids_l) + len(cases[0].ids_r) == n_l + n_r
    with Handles(1) as (mt,):
        mt.set_map(cases[0].map_ids, cases[0].map_pw)
        single = [_single(mt, c) for c in cases]
        mb = MotionBatch([mt] * len(cases))
        _same(mb.track_motion([_frame(c) for c in cases]), single)
        mb.close()


def test_forcing_the_large_cap_changes_no_bit(gpu, monkeypatch):
    """RSVIO_PNP_BATCH_CAP is read by every run, so both legs run in this process."""
    from rsvio.motion import MotionBatch, RansacConfig
    cases = [_count_slice(300, 300), PC.get("count", "n64+64"), PC.get("count", "n1+1")]
    with Handles(1) as (mt,):
        mt.set_map(cases[0].map_ids, cases[0].map_pw)
        mb = MotionBatch([mt] * len(cases))
        frames = [_frame(c) for c in cases]
        rc = RansacConfig(n_hyp=8, seed=3)
        monkeypatch.delenv("RSVIO_PNP_BATCH_CAP", raising=False)
        a, ar = mb.track_motion(frames), mb.track_motion_robust(frames, rc, want_counts=True)
        monkeypatch.setenv("RSVIO_PNP_BATCH_CAP", "4096")
        b, br = mb.track_motion(frames), mb.track_motion_robust(frames, rc, want_counts=True)
        monkeypatch.delenv("RSVIO_PNP_BATCH_CAP")
        assert [_bits(x) for x in a] == [_bits(x) for x in b]
        _same(a, [_single(mt, c) for c in cases])
        for x, y in zip(ar, br):
            _same_robust(x, y)
        mb.close()


# ---------------------------------------------------------------- 4. more workgroups than CUs

def test_more_workgroups_than_cus(gpu):
    from rsvio.motion import MotionBatch
    names = ["tiny-1", "tiny-2", "tiny-3", "clean", "tiny-1-left-only"]
    handle_of = [0, 1, 2, 3, 0]   # tiny-1-left-only is tiny-1's frame without its right list: the same map
    cases = [PC.get("lm", n) for n in names]
    with Handles(4) as mts:
        for c, k in zip(cases[:4], handle_of):
            mts[k].set_map(c.map_ids, c.map_pw)
        assert np.array_equal(cases[4].map_ids, cases[0].map_ids)
        single = [_single(mts[k], c) for c, k in zip(cases, handle_of)]
        n = 300
        mb = MotionBatch([mts[handle_of[i % 5]] for i in range(n)])
        frames = [_frame(c) for c in cases]
        out = mb.track_motion([frames[i % 5] for i in range(n)])
        _same(out, [single[i % 5] for i in range(n)])
        mb.close()


# ---------------------------------------------------------------- 5. maps follow the handles

def test_maps_follow_the_handles(gpu):
    """set_map between runs -- a larger table, a smaller one, an empty map -- is picked up by the
    slot of that handle; the other slots (a map with the id 2^64 - 1 beside the table, a map whose
    lookups walk ten buckets) do not change."""
    from rsvio.motion import MotionBatch, MotionFrame
    top, run = PC.get("join", "top-id"), PC.get("join", "collide-full")
    m, maps = PC.remap_sequence()
    with Handles(3) as (a, b, c):
        a.set_map(top.map_ids, top.map_pw)
        c.set_map(run.map_ids, run.map_pw)
        assert a.map_stats()["has_top"] == 1 and c.map_stats()["max_probe"] > 1
        sa, sc = _single(a, top), _single(c, run)
        mb = MotionBatch([a, b, c])
        frames = [_frame(top), MotionFrame(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2), _frame(run)]
        n_obs = []
        for label, ids, pw in maps:
            b.set_map(ids, pw)
            sb = b.track_motion(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2)
            _same(mb.track_motion(frames), [sa, sb, sc])
            n_obs.append(sb.n_observations)
        assert n_obs[0] == n_obs[3] > 1500 and n_obs[1] == 80 and n_obs[2] == 0
        mb.close()


# ---------------------------------------------------------------- 6. device-resident lists

def test_device_resident_lists(gpu):
    """One slot's ids at stride 24 in a device buffer and its uv as device tensors, read in place."""
    import torch

    from rsvio.motion import MotionBatch, MotionFrame, pnp_cfg
    cases = [PC.get("lm", "clean"), PC.get("lm", "big-rot-A"), PC.get("lm", "tiny-3")]
    with Handles(3) as mts:
        for mt, c in zip(mts, cases):
            mt.set_map(c.map_ids, c.map_pw)
        mb = MotionBatch(mts)
        host = mb.track_motion([_frame(c) for c in cases])
        c = cases[1]
        dev = {}
        for s in ("l", "r"):
            ids = np.ascontiguousarray(getattr(c, "ids_" + s), np.uint64)
            buf = np.full((len(ids), 24), 0xEE, np.uint8)
            buf[:, :8] = ids.view(np.uint8).reshape(-1, 8)
            dev["ids_" + s] = torch.from_numpy(buf.reshape(-1)).cuda()
            dev["uv_" + s] = torch.from_numpy(np.ascontiguousarray(getattr(c, "uv_" + s), np.float32)).cuda()
        torch.cuda.synchronize()
        frames = [_frame(cases[0]),
                  MotionFrame(dev["ids_l"], dev["uv_l"], dev["ids_r"], dev["uv_r"], c.T_last, c.T_C_B2,
                              cfg=pnp_cfg(**c.cfg), on_device=True, id_stride=24),
                  _frame(cases[2])]
        mixed = mb.track_motion(frames)
        _same(mixed, host)
        _same(mixed, [_single(mt, k) for mt, k in zip(mts, cases)])
        assert mixed[1].status == 3 and mixed[1].iterations == 10
        mb.close()


# ---------------------------------------------------------------- 7. robust

def _same_robust(b, s, masks=True, counts=True):
    assert _bits(b.motion) == _bits(s.motion)
    assert (b.ransac_status, b.n_pairs, b.n_valid_pairs, b.n_valid_hyp, b.best_hyp, b.best_count, b.n_inliers) == \
        (s.ransac_status, s.n_pairs, s.n_valid_pairs, s.n_valid_hyp, s.best_hyp, s.best_count, s.n_inliers)
    if masks:
        assert np.array_equal(b.mask_l, s.mask_l) and np.array_equal(b.mask_r, s.mask_r)
    else:
        assert b.mask_l is None and b.mask_r is None
    if counts:
        assert np.array_equal(b.hyp_count, s.hyp_count)
    else:
        assert b.hyp_count is None
    assert b.device_ms > 0.0 and b.motion.kernel_ms > 0.0


def _robust_inputs():
    """(frame-like with its map, uv_l, uv_r) per slot: two corrupted frames, a clean one, one with two
    pairs only, one with 8 joined observations (below min_inliers = 10) and one for explicit samples."""
    from rsvio import synthetic as S
    out = []
    for seed in (1234, 77):
        m, uv_l, uv_r, _, _ = R.corrupted_frame(rng_seed=seed)
        out.append(dataclasses.replace(m, uv_l=uv_l, uv_r=uv_r))
    out.append(S.motion_frame(n_map=400, n_feat=120, noise_px=0.3, map_noise=0.001, seed=3))
    few = Scene(_points(12), step=(0.01, 0.005))
    few.ids_r = few.ids_r.copy()
    few.ids_r[2:12] += np.uint64(7 * 10 ** 6)
    out.append(few)
    out.append(Scene(_points(4, seed=3), step=(0.01, 0.005)))
    out.append(S.motion_frame(n_map=400, n_feat=120, noise_px=0.3, map_noise=0.001, seed=21, outlier_frac=0.1))
    return out


@pytest.fixture(scope="module")
def robust_setup(gpu):
    from rsvio.motion import MotionBatch
    ins = _robust_inputs()
    with Handles(len(ins)) as mts:
        for mt, m in zip(mts, ins):
            mt.set_map(m.map_ids, m.map_pw)
        mb = MotionBatch(mts)
        yield mts, mb, ins
        mb.close()


@pytest.mark.parametrize("n_hyp", [1, 8, 256])
def test_robust_batch_equals_the_single_calls(robust_setup, n_hyp):
    from rsvio.motion import MotionFrame, RansacConfig, pnp_cfg
    mts, mb, ins = robust_setup
    rc = RansacConfig(n_hyp=n_hyp, seed=R.CORRUPT_SEED, inlier_sq_error=R.CORRUPT_SQ, min_inliers=10)
    lm = pnp_cfg(**R.CORRUPT_LM)
    rng = np.random.default_rng(5)
    samples = [None] * len(ins)
    samples[5] = np.stack([rng.choice(120, 3, replace=False) for _ in range(n_hyp)]).astype(np.int32)
    single = [mt.track_motion_robust(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2, rc, cfg=lm,
                                     samples=s, want_counts=True) for mt, m, s in zip(mts, ins, samples)]
    assert single[3].n_pairs == 2 and single[3].ransac_status == 2 and single[3].motion.success
    assert single[4].ransac_status == -1 and single[4].best_count <= 8 and single[4].motion.status == -2
    assert single[5].n_pairs == 120
    if n_hyp == 256:
        assert all(s.ransac_status == 1 and s.motion.success and s.best_hyp > 0 for s in single[:2])
    frames = [MotionFrame(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2, samples=s)
              for m, s in zip(ins, samples)]
    out = mb.track_motion_robust(frames, rc, cfg=lm, want_counts=True)
    for b, s in zip(out, single):
        _same_robust(b, s)
    # NULL masks and counts in some slots
    wm = [True, False, True, False, False, True]
    wc = [False, True, False, False, True, True]
    part = mb.track_motion_robust(frames, rc, cfg=lm, want_counts=wc, want_masks=wm)
    for b, s, m_, c_ in zip(part, single, wm, wc):
        _same_robust(b, s, masks=m_, counts=c_)


def test_robust_collapse_and_plain_after_robust(robust_setup):
    """One hypothesis accepting everything is the plain batch bit for bit; the plain run follows a
    robust run on the same batch."""
    from rsvio.motion import MotionFrame, RansacConfig
    mts, mb, ins = robust_setup
    frames = [MotionFrame(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2) for m in ins]
    rob = mb.track_motion_robust(frames, RansacConfig(n_hyp=1, inlier_sq_error=1e300, min_inliers=1))
    plain = mb.track_motion(frames)
    assert [_bits(r.motion) for r in rob] == [_bits(p) for p in plain]
    assert all(r.best_hyp == 0 and r.best_count == p.n_observations == r.n_inliers for r, p in zip(rob, plain))
    _same(plain, [mt.track_motion(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2)
                  for mt, m in zip(mts, ins)])


def test_robust_argument_errors(robust_setup):
    from rsvio import RsvioError
    from rsvio.motion import MotionFrame, RansacConfig
    mts, mb, ins = robust_setup
    frames = [MotionFrame(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2) for m in ins]
    for bad in (dict(n_hyp=0), dict(n_hyp=1025), dict(inlier_sq_error=0.0)):
        with pytest.raises(RsvioError) as e:
            mb.track_motion_robust(frames, RansacConfig(**bad))
        assert e.value.code == -1
