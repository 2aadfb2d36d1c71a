"""Batched process_frame on the GPU (rsvio_tracker_batch_*: TrackerBatch): one stereo frame per
tracker handle, n handles per call.  The reference of every assertion is the single-stream
process_frame on a twin handle fed the same images; the comparison is array_equal on the raw bytes of
both lists plus n_l, n_r and the status.

Shapes: 160 x 120, 2 levels, grid 16, 20 iterations, threshold 0.01 (96 x 64 where many streams or
small lists are wanted).  Sequences A = stereo_sequence(7, 160, 120, seed=1) and
B = stereo_sequence(3, 160, 120, seed=2), rendered once per module, and what the CPU oracle gives
for them (left/right features, tracks lost):
  plain A                                 39/39 on the first frame, none lost afterwards
  [A0, A1, half(A2|B2), A3]               39/39, 39/39, 37/38 with 21 lost, 40/41 with 18 lost
  [A0, A1, (A2.left, B2.right), A3]       right lists of 1 and 3 against left lists of 39 and 42
  [A0, flat 77, A1, A2]                   39/39 -> 0/0, all 39 lost -> 37/37 with new ids from 39 up
  [flat, A0, A1, A2]                      starts at 0/0
  [A0, A1, B2, B1]                        loses 38 of 39 and re-detects
  96 x 64 (seeds 3, 4, 5)                 8 to 12 features
Each test asserts the property it relies on (0 < lost < n, n_l != n_r, an empty list) on the
single-stream result, so a case cannot quietly turn trivial."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 160, 120
PARAMS = dict(levels=2, grid_size=16, optical_flow_max_iterations=20, optical_flow_convergence_threshold=0.01)
CAPACITY = -4


def _tracker(gpu, w=W, h=H, **kw):
    return gpu.StereoPatchTracker(w, h, **{**PARAMS, **kw})


def _single(trk, left, right):
    """process_frame on one handle through the C ABI: (left list, right list, status)."""
    from rsvio import _lib
    from rsvio._lib import ptr
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    nl, nr = C.c_size_t(0), C.c_size_t(0)
    rc = _lib.load().rsvio_tracker_process_frame(trk._h, ptr(left), ptr(right), trk.width, ptr(trk._out_l), trk.cap,
                                                 C.byref(nl), ptr(trk._out_r), trk.cap, C.byref(nr))
    assert rc in (0, CAPACITY), rc
    trk._n = (nl.value, nr.value)
    return trk._out_l[:nl.value].copy(), trk._out_r[:nr.value].copy(), rc


def _same(batch, single, what=""):
    (bl, br, bs), (sl, sr, ss) = batch, single
    assert (len(bl), len(br), bs) == (len(sl), len(sr), ss), what
    assert np.array_equal(bl.view(np.uint8), sl.view(np.uint8)), what
    assert np.array_equal(br.view(np.uint8), sr.view(np.uint8)), what


def _lost(prev, cur):
    return len(set(prev["id"].tolist()) - set(cur["id"].tolist()))


class Seqs:
    """The rendered sequences and, per sequence, the single-stream result of every frame (a twin
    handle run once and shared; never modified)."""

    def __init__(self, gpu):
        from rsvio import synthetic as S
        A = list(S.stereo_sequence(7, W, H, seed=1))
        B = list(S.stereo_sequence(3, W, H, seed=2))
        flat = np.full((H, W), 77, np.uint8)

        def half(a, b):
            o = a.copy()
            o[:, 80:] = b[:, 80:]
            return o

        self.A, self.B, self.flat = A, B, flat
        self.frames = {
            "plain": A[:4],
            "half": [A[0], A[1], (half(A[2][0], B[2][0]), half(A[2][1], B[2][1])), A[3]],
            "mixlr": [A[0], A[1], (A[2][0], B[2][1]), A[3]],
            "flatmid": [A[0], (flat, flat), A[1], A[2]],
            "flatfirst": [(flat, flat), A[0], A[1], A[2]],
            "swap": [A[0], A[1], B[2], B[1]],
            "late1": A[1:5], "late2": A[2:6], "late3": A[3:7],
        }
        self.names = list(self.frames)
        self.gpu = gpu
        self.ref = {k: self.run_single(v) for k, v in self.frames.items()}
        # the properties the cases rely on
        r = self.ref
        assert [len(x[0]) for x in r["plain"]][:3] == [39, 39, 39] and _lost(r["plain"][0][0], r["plain"][3][0]) == 0
        n, lost = len(r["half"][1][0]), _lost(r["half"][1][0], r["half"][2][0])
        assert 0 < lost < n and len(r["half"][2][0]) != len(r["half"][2][1])
        assert len(r["mixlr"][2][1]) < len(r["mixlr"][2][0]) and len(r["mixlr"][3][1]) < len(r["mixlr"][3][0])
        assert len(r["flatmid"][1][0]) == 0 and len(r["flatmid"][1][1]) == 0
        assert int(r["flatmid"][2][0]["id"].min()) == len(r["flatmid"][0][0]) > 0
        assert len(r["flatfirst"][0][0]) == 0 and len(r["flatfirst"][1][0]) > 0
        assert _lost(r["swap"][1][0], r["swap"][2][0]) > 30 and len(r["swap"][2][0]) > 30
        assert all(s == 0 for v in r.values() for _, _, s in v)

    def run_single(self, frames, **kw):
        t = _tracker(self.gpu, **kw)
        out = [_single(t, l, r) for l, r in frames]
        t.close()
        return out


@pytest.fixture(scope="module")
def seqs(gpu):
    return Seqs(gpu)


def _run_batch(gpu, seqs, names, n_frames=4):
    """One batch over fresh handles, stream i on sequence names[i]; [[(l, r, status) per slot] per frame]."""
    ts = [_tracker(gpu) for _ in names]
    tb = gpu.TrackerBatch(ts)
    out = []
    for k in range(n_frames):
        res = tb.process_frames([seqs.frames[s][k][0] for s in names], [seqs.frames[s][k][1] for s in names])
        assert tb.device_ms > 0.0
        out.append([(l, r, st) for (l, r), st in zip(res, tb.status)])
        for t, (l, _r) in zip(ts, res):   # the cached lists follow the batch
            assert sorted(t.get_track_points()[0]) == l["id"].tolist()
    tb.close()
    for t in ts:
        t.close()
    return out


# ---------------------------------------------------------------- 1. n streams on different sequences

@pytest.mark.parametrize("n", [1, 2, 5, 9])
def test_streams_equal_their_single_calls(gpu, seqs, n):
    """n = 5 passes the 4-batch limit of the by-value LK launch, n = 5 and 9 the 8-image limit of
    the by-pointer pyramid launch; every stream is on its own sequence."""
    names = (seqs.names[1:] + seqs.names[:1])[:n] if n < 9 else seqs.names
    assert len(set(names)) == n
    out = _run_batch(gpu, seqs, names)
    for k, frame in enumerate(out):
        for i, s in enumerate(names):
            _same(frame[i], seqs.ref[s][k], f"frame {k} slot {i} ({s})")


# ---------------------------------------------------------------- 2. 40 small streams

def test_forty_small_streams(gpu):
    from rsvio import synthetic as S
    w, h = 96, 64
    rendered = [list(S.stereo_sequence(5, w, h, seed=s)) for s in (3, 4, 5)]
    ref = {}
    for q in range(3):
        for start in range(3):
            t = _tracker(gpu, w, h)
            ref[q, start] = [_single(t, *rendered[q][start + k]) for k in range(3)]
            t.close()
    assert all(7 <= len(l) <= 13 for v in ref.values() for l, _, _ in v)
    n = 40
    which = [(i % 3, (i // 3) % 3) for i in range(n)]
    ts = [_tracker(gpu, w, h) for _ in range(n)]
    tb = gpu.TrackerBatch(ts)
    for k in range(3):
        res = tb.process_frames([rendered[q][s + k][0] for q, s in which], [rendered[q][s + k][1] for q, s in which])
        for i, (q, s) in enumerate(which):
            _same((*res[i], tb.status[i]), ref[q, s][k], f"frame {k} slot {i}")
    tb.close()
    for t in ts:
        t.close()


# ---------------------------------------------------------------- 3. run to run

def test_run_to_run(gpu, seqs):
    names = ["half", "plain", "swap"]
    a, b = _run_batch(gpu, seqs, names), _run_batch(gpu, seqs, names)
    for fa, fb in zip(a, b):
        for x, y in zip(fa, fb):
            _same(x, y)


# ---------------------------------------------------------------- 4. mixed history

def test_streams_join_a_running_batch(gpu, seqs):
    """Two streams join at the third call: first-frame slots and tracked slots share one launch."""
    old, new = ["half", "flatmid"], ["plain", "mixlr"]
    ts = [_tracker(gpu) for _ in range(4)]
    tb = gpu.TrackerBatch(ts[:2])
    for k in range(2):
        res = tb.process_frames([seqs.frames[s][k][0] for s in old], [seqs.frames[s][k][1] for s in old])
        for i, s in enumerate(old):
            _same((*res[i], tb.status[i]), seqs.ref[s][k])
    tb.close()
    tb = gpu.TrackerBatch([ts[2], ts[0], ts[3], ts[1]])
    order = [("plain", 0), ("half", 2), ("mixlr", 0), ("flatmid", 2)]
    for step in range(2):
        fr = [seqs.frames[s][k + step] for s, k in order]
        res = tb.process_frames([f[0] for f in fr], [f[1] for f in fr])
        for i, (s, k) in enumerate(order):
            _same((*res[i], tb.status[i]), seqs.ref[s][k + step], f"step {step} slot {i}")
    tb.close()
    for t in ts:
        t.close()


# ---------------------------------------------------------------- 5. batch and single calls alternate

def test_batch_and_single_calls_alternate_on_a_handle(gpu, seqs):
    ts = [_tracker(gpu), _tracker(gpu)]
    tb = gpu.TrackerBatch(ts)
    names = ["half", "swap"]
    for k in range(4):
        fr = [seqs.frames[s][k] for s in names]
        if k % 2 == 0:
            res = tb.process_frames([f[0] for f in fr], [f[1] for f in fr])
            got = [(*res[i], tb.status[i]) for i in range(2)]
        else:
            got = [_single(t, *f) for t, f in zip(ts, fr)]
        for i, s in enumerate(names):
            _same(got[i], seqs.ref[s][k], f"frame {k} slot {i}")
    tb.close()
    for t in ts:
        t.close()


# ---------------------------------------------------------------- 6. remove_id between batch calls

def test_remove_id_between_batch_calls(gpu, seqs):
    fr = seqs.frames["plain"]
    twin = _tracker(gpu)
    ts = [_tracker(gpu), _tracker(gpu)]
    tb = gpu.TrackerBatch(ts)
    sl, _sr, _ = _single(twin, *fr[0])
    res = tb.process_frames([fr[0][0]] * 2, [fr[0][1]] * 2)
    drop = sl["id"][::3]
    assert 0 < len(drop) < len(sl)
    twin.remove_id(drop)
    ts[0].remove_id(drop)
    assert ts[0].get_track_points() == twin.get_track_points()
    for k in (1, 2):
        s = _single(twin, *fr[k])
        res = tb.process_frames([fr[k][0]] * 2, [fr[k][1]] * 2)
        _same((*res[0], tb.status[0]), s, f"frame {k}")
        _same((*res[1], tb.status[1]), seqs.ref["plain"][k], f"frame {k} (untouched slot)")
        assert not set(drop.tolist()) & set(res[0][0]["id"].tolist())
    tb.close()
    for t in ts + [twin]:
        t.close()


# ---------------------------------------------------------------- 7. capacity

def test_slot_capacity_does_not_fail_the_call(gpu, seqs):
    """max_features = 16 against 39 new points: that slot reports RSVIO_ERR_CAPACITY with the twin's
    lists; a flat slot and a slot with 10 features are OK; the next frame equals the twin's too."""
    A = seqs.A
    corner = A[0][0].copy()
    corner[:, 48:] = 77
    frames = [[A[0], A[1]], [(seqs.flat, seqs.flat), A[1]], [(corner, corner), A[1]]]
    ref = [seqs.run_single(f, max_features=16) for f in frames]
    assert ref[0][0][2] == CAPACITY and len(ref[0][0][0]) == 16
    assert ref[1][0][2] == 0 and len(ref[1][0][0]) == 0
    assert ref[2][0][2] == 0 and 0 < len(ref[2][0][0]) < 16
    ts = [_tracker(gpu, max_features=16) for _ in frames]
    tb = gpu.TrackerBatch(ts)
    for k in range(2):
        res = tb.process_frames([f[k][0] for f in frames], [f[k][1] for f in frames])   # does not raise
        for i in range(3):
            _same((*res[i], tb.status[i]), ref[i][k], f"frame {k} slot {i}")
    tb.close()
    for t in ts:
        t.close()


def test_output_capacity_and_lists_not_copied(gpu):
    """cap_l smaller than the list: truncation and CAPACITY as the single call; out_l NULL with
    capacity 0: OK, n_l reported, nothing copied."""
    from rsvio import _lib
    from rsvio import synthetic as S
    from rsvio._lib import ptr
    w, h = 96, 64
    left, right = next(iter(S.stereo_sequence(1, w, h, seed=3)))
    twin = _tracker(gpu, w, h)
    sl, sr, st = _single(twin, left, right)
    assert st == 0 and len(sl) > 3 and len(sr) > 3
    small = _tracker(gpu, w, h)
    nl, nr = C.c_size_t(0), C.c_size_t(0)
    rc = _lib.load().rsvio_tracker_process_frame(small._h, ptr(left), ptr(right), w, ptr(small._out_l), 3,
                                                 C.byref(nl), ptr(small._out_r), small.cap, C.byref(nr))
    assert rc == CAPACITY and nl.value == 3 and nr.value == len(sr)
    ts = [_tracker(gpu, w, h) for _ in range(3)]
    tb = gpu.TrackerBatch(ts)
    tab, keep = tb._frames([left] * 3, [right] * 3)
    tab[0].cap_l = 3
    tab[1].out_l, tab[1].cap_l = None, 0
    guard = ts[1]._out_l.copy()
    assert _lib.load().rsvio_tracker_batch_process_frames(tb._h, C.addressof(tab), None) == 0   # device_ms NULL
    assert (tab[0].status, tab[0].n_l, tab[0].n_r) == (CAPACITY, 3, len(sr))
    assert np.array_equal(ts[0]._out_l[:3].view(np.uint8), sl[:3].view(np.uint8))
    assert np.array_equal(ts[0]._out_r[:len(sr)].view(np.uint8), sr.view(np.uint8))
    assert (tab[1].status, tab[1].n_l, tab[1].n_r) == (0, len(sl), len(sr))
    assert np.array_equal(ts[1]._out_l, guard)
    assert np.array_equal(ts[1]._out_r[:len(sr)].view(np.uint8), sr.view(np.uint8))
    assert (tab[2].status, tab[2].n_l, tab[2].n_r) == (0, len(sl), len(sr))
    assert np.array_equal(ts[2]._out_l[:len(sl)].view(np.uint8), sl.view(np.uint8))
    del keep
    tb.close()
    for t in ts + [twin, small]:
        t.close()


# ---------------------------------------------------------------- 8. cameras

def test_undistorted_after_a_batch_call(gpu, seqs):
    from rsvio.camera import EUROC
    names = ["plain", "half"]
    twins, ts = [_tracker(gpu) for _ in names], [_tracker(gpu) for _ in names]
    for t in twins + ts:
        t.set_cameras(*EUROC)
    tb = gpu.TrackerBatch(ts)
    for k in range(3):
        fr = [seqs.frames[s][k] for s in names]
        res = tb.process_frames([f[0] for f in fr], [f[1] for f in fr])
        for i, s in enumerate(names):
            _same((*res[i], tb.status[i]), _single(twins[i], *fr[i]), f"frame {k} slot {i}")
            ul, ur = ts[i].undistorted()
            tl, tr = twins[i].undistorted()
            assert len(ul) == len(res[i][0]) > 0 and len(ur) == len(res[i][1])
            assert np.array_equal(ul.view(np.uint32), tl.view(np.uint32))
            assert np.array_equal(ur.view(np.uint32), tr.view(np.uint32))
    tb.close()
    for t in twins + ts:
        t.close()


# ---------------------------------------------------------------- 9. device images and strided host images

def test_device_images_and_strided_host_images(gpu, seqs):
    import torch
    names = ["half", "plain", "swap"]
    ts = [_tracker(gpu) for _ in names]
    tb = gpu.TrackerBatch(ts)
    for k in range(4):
        lefts, rights, keep = [], [], []
        for i, s in enumerate(names):
            l, r = seqs.frames[s][k]
            if i == 1:   # device tensors
                l, r = torch.from_numpy(np.ascontiguousarray(l)).cuda(), torch.from_numpy(np.ascontiguousarray(r)).cuda()
            elif i == 2:   # rows 208 bytes apart
                wide = np.full((2, H, W + 48), 0xEE, np.uint8)
                wide[0, :, :W], wide[1, :, :W] = l, r
                l, r = wide[0, :, :W], wide[1, :, :W]
                assert l.strides == (W + 48, 1)
            lefts.append(l)
            rights.append(r)
        torch.cuda.synchronize()
        tab, _keep = tb._frames(lefts, rights)
        assert [int(c.on_device) for c in tab] == [0, 1, 0] and [int(c.stride) for c in tab] == [W, 0, W + 48]
        res = tb.process_frames(lefts, rights)
        for i, s in enumerate(names):
            _same((*res[i], tb.status[i]), seqs.ref[s][k], f"frame {k} slot {i}")
    tb.close()
    for t in ts:
        t.close()


# ---------------------------------------------------------------- 10. tracker -> PnP in batch

def test_tracker_to_pnp_chain_on_the_device(gpu, seqs):
    """The batch's lists handed to MotionBatch in place (device_lists, id_stride = 32): per slot the
    result equals track_motion_tracker on the same handle."""
    from rsvio import _lib
    from rsvio import synthetic as S
    from rsvio.camera import EUROC
    from rsvio.motion import MotionBatch, MotionFrame, MotionTracker
    from test_motion_edges_gpu import _bits
    names = ["plain", "half", "late1"]
    ts = [_tracker(gpu) for _ in names]
    mts = [MotionTracker() for _ in names]
    for t in ts:
        t.set_cameras(*EUROC)
    tb = gpu.TrackerBatch(ts)
    T_last = np.eye(4)
    T_C_B2 = np.stack([np.linalg.inv(S.T_B_CL).reshape(16), np.linalg.inv(S.T_B_CR).reshape(16)])
    res = tb.process_frames([seqs.frames[s][0][0] for s in names], [seqs.frames[s][0][1] for s in names])
    for t, mt, (fl, _fr) in zip(ts, mts, res):   # a map from the first frame's features at depth 2
        ul, _ur = t.undistorted()
        rays = np.concatenate([ul.astype(np.float64), np.ones((len(ul), 1))], 1) * 2.0
        p_W = (S.T_B_CL[:3, :3] @ rays.T).T + S.T_B_CL[:3, 3]
        mt.set_map(fl["id"].astype(np.uint64), p_W.astype(np.float32))
    mb = MotionBatch(mts)
    for k in (1, 2):
        res = tb.process_frames([seqs.frames[s][k][0] for s in names], [seqs.frames[s][k][1] for s in names])
        frames = []
        for t, (fl, fr) in zip(ts, res):
            d_l, n_l, d_r, n_r, u_l, u_r = t.device_lists()
            assert (n_l, n_r) == (len(fl), len(fr)) and d_l and d_r and u_l and u_r
            frames.append(MotionFrame(d_l, u_l, d_r, u_r, T_last, T_C_B2, on_device=True,
                                      id_stride=C.sizeof(_lib.Feature), n_l=n_l, n_r=n_r))
        out = mb.track_motion(frames)
        for i, (t, mt) in enumerate(zip(ts, mts)):
            one = mt.track_motion_tracker(t, T_last, T_C_B2)
            assert _bits(out[i]) == _bits(one), f"frame {k} slot {i}"
            assert one.n_observations > 20
    mb.close()
    tb.close()
    for t in ts + mts:
        t.close()
    plain = _tracker(gpu)   # without cameras: no undistorted lists
    _single(plain, *seqs.frames["plain"][0])
    d = plain.device_lists()
    assert d[1] == d[3] == 39 and d[0] and d[2] and d[4] is None and d[5] is None
    plain.close()


# ---------------------------------------------------------------- 11. refusals

def test_refusals_leave_every_handle_usable(gpu, seqs):
    from rsvio import RsvioError, _lib
    fr = seqs.frames["half"]
    ts = [_tracker(gpu) for _ in range(3)]
    other = _tracker(gpu, grid_size=20)
    for bad in ([ts[0], ts[1], ts[0]], [ts[0], other]):
        with pytest.raises(RsvioError) as e:
            gpu.TrackerBatch(bad)
        assert e.value.code == -1 and f"slot {len(bad) - 1}" in str(e.value)
    tb = gpu.TrackerBatch(ts)
    res = tb.process_frames([fr[0][0]] * 3, [fr[0][1]] * 3)
    for i in range(3):
        _same((*res[i], tb.status[i]), seqs.ref["half"][0])
    # a submitted, uncollected frame on slot 1
    ts[1].submit(*fr[1])
    with pytest.raises(RsvioError) as e:
        tb.process_frames([fr[1][0]] * 3, [fr[1][1]] * 3)
    assert e.value.code == -1 and "slot 1" in str(e.value)
    l, r = ts[1].collect()
    _same((l, r, 0), seqs.ref["half"][1])
    for i in (0, 2):
        _same(_single(ts[i], *fr[1]), seqs.ref["half"][1])
    # a NULL image in slot 2, a host stride below the width in slot 0: nothing written
    for k, change in ((2, lambda c: setattr(c, "right", None)), (0, lambda c: setattr(c, "stride", W - 1))):
        tab, keep = tb._frames([fr[2][0]] * 3, [fr[2][1]] * 3)
        change(tab[k])
        for c in tab:
            c.status, c.n_l = 77, 12345
        assert _lib.load().rsvio_tracker_batch_process_frames(tb._h, C.addressof(tab), None) == -1
        assert f"slot {k}" in _lib.load().rsvio_last_error().decode()
        assert all((c.status, c.n_l) == (77, 12345) for c in tab)
    res = tb.process_frames([fr[2][0]] * 3, [fr[2][1]] * 3)
    for i in range(3):
        _same((*res[i], tb.status[i]), seqs.ref["half"][2], f"slot {i}")
    tb.close()
    for t in ts + [other]:
        t.close()
