"""The batched keyframe step (rsvio_ba_batch_run_active / _triangulate / _check_landmarks /
_covariance, BundleBatch's methods and WindowBatch): every slot of a batched call against the single
call on a twin handle (or the same handle) bit for bit, one slot per path also against the numpy /
oracle references of the single calls' suites, subsets, refusals and the SlidingWindow mirror.

Windows: the sizes the single calls' suites use as the smallest that reach each path -- (2, 30) and
(3, 40), (5, 90), (10, 200), (11, 200) (9 and 10 free keyframes: the panel solver's last two
templates), (12, 200) (11 free keyframes: the block solver's first template, padded to 13), a
20-keyframe pattern window (the block solver's largest) -- and
the triangulation suite's 4-keyframe window on the depth-2 ray, whose numpy reference is known."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import test_ba_triangulate_gpu as TT
import test_covariance_gpu as TC

pytestmark = pytest.mark.gpu

SIZES = [(2, 30), (3, 40), (5, 90), (10, 200), (11, 200), (12, 200)]


@functools.lru_cache(maxsize=None)
def _small():
    from rsvio import synthetic as S
    p = S.ba_problem(n_kf=4, n_lm=130, kf_per_lm=3)
    return dataclasses.replace(p, p_W=TT._ray_start(p))


@functools.lru_cache(maxsize=None)
def _mixed():
    """The mixed batch: the triangulation suite's window, the sizes, the 20-keyframe window."""
    return [_small()] + [TC._size_problem(*s) for s in SIZES] + [TC._pattern_problem("staircase")]


def _handles(probs):
    return [TC._adjuster(p) for p in probs]


def _close(*things):
    for t in things:
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            x.close()


def _same_state(a, b):
    sa, sb = a.state(), b.state()
    return sa[0].tobytes() == sb[0].tobytes() and sa[1].tobytes() == sb[1].tobytes()


def _same_result(a, b):
    return (a.status, a.iterations, a.initial_cost, a.final_cost) == (b.status, b.iterations, b.initial_cost,
                                                                      b.final_cost)


def _same_cov(a, b):
    """Every field of two Covariance results but the timing, bit for bit."""
    if (a.status, a.n_free, a.n_singular, a.cost) != (b.status, b.n_free, b.n_singular, b.cost):
        return False
    for x, y in ((a.pose, b.pose), (a.full, b.full), (a.landmarks, b.landmarks), (a.flags, b.flags)):
        if (x is None) != (y is None) or (x is not None and x.tobytes() != y.tobytes()):
            return False
    return True


def _masks(probs):
    """A mask on every other slot (about two thirds of its landmarks), none on the rest."""
    rng = np.random.default_rng(31)
    return [(rng.random(p.n_lm) < 0.66).astype(np.uint8) if i % 2 else None for i, p in enumerate(probs)]


# ------------------------------------------------------------------------------------------
# 1: triangulate, slot against the single call
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [TT.ALL_VIEWS, TT.FIRST_STEREO])
def test_triangulate_slots_equal_the_single_call(gpu, mode):
    from rsvio.ba import BundleBatch
    probs = _mixed() + [_small()]
    masks = _masks(probs)
    masks[0] = masks[-1] = None
    # the last slot is the first slot's window under a tighter gate (depths span 1.6 .. 10 m); slot
    # 2 has no gate of its own: it takes the call's
    gates = [TT._gate(mode) for _ in probs]
    gates[2] = None
    gates[-1] = TT._gate(mode, 0.1, 4.0)
    wins, twins = _handles(probs), _handles(probs)
    batch = BundleBatch(wins)
    got = batch.triangulate(masks, gates, want=True)
    assert batch.device_ms > 0.0
    for i, (tw, m, g) in enumerate(zip(twins, masks, gates)):
        pw, info, n = tw.triangulate(m, g, want=True)
        assert np.array_equal(got[i][0], pw) and got[i][1].tobytes() == info.tobytes() and got[i][2] == n, i
        assert np.array_equal(info["flags"] == TT.NOT_SELECTED, np.zeros(len(info), bool) if m is None else m == 0)
    # the numpy reference of the single call's suite on slot 0; the two gates of one call
    TT._assert_tri(got[0], TT._np_landmarks(_small(), TT._gate(mode)))
    assert np.all(got[0][1]["flags"] == TT.OK)
    tight = got[-1][1]["flags"]
    assert (tight & TT.DEPTH).any() and (tight == TT.OK).any()
    TT._assert_tri(got[-1], TT._np_landmarks(_small(), gates[-1]))
    again = batch.triangulate(masks, gates, want=True)           # idempotent and deterministic
    assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(got, again))
    _close(batch, wins, twins)


# ------------------------------------------------------------------------------------------
# 2: the enqueue-only triangulate in front of a batch run and of single runs
# ------------------------------------------------------------------------------------------
def test_enqueue_only_triangulate_then_runs(gpu):
    from rsvio.ba import BundleBatch
    probs = _mixed()
    masks, gate = _masks(probs), TT._gate(TT.ALL_VIEWS)
    every = [True] * len(probs)
    # batched triangulate + run_active against single triangulates + the batch run: one launch chain
    wins, twins = _handles(probs), _handles(probs)
    batch, tbatch = BundleBatch(wins), BundleBatch(twins)
    assert batch.triangulate(masks, gate) == [None] * len(probs)
    res = batch.run(active=every)
    for tw, m in zip(twins, masks):
        tw.triangulate(m, gate)
    tres = tbatch.run()
    for i in range(len(probs)):
        assert _same_result(res[i], tres[i]) and _same_state(wins[i], twins[i]), i
    assert res[0].status > 0 and res[0].iterations >= 1
    _close(batch, tbatch, wins, twins)
    # batched triangulate, then each handle's own run on its own stream
    wins, twins = _handles(probs), _handles(probs)
    batch = BundleBatch(wins)
    batch.triangulate(masks, gate)
    for i, (w, tw, m) in enumerate(zip(wins, twins, masks)):
        r = w.run()
        tw.triangulate(m, gate)
        assert _same_result(r, tw.run()) and _same_state(w, tw), i
    _close(batch, wins, twins)


# ------------------------------------------------------------------------------------------
# 3: check
# ------------------------------------------------------------------------------------------
def _swapped(small):
    """test_check_landmarks' window: landmark 7's left and right observations swapped."""
    bad = dataclasses.replace(small, obs_uv=small.obs_uv.copy())
    mine = np.nonzero(small.obs_lm == 7)[0]
    for a in mine:
        b = [i for i in mine if small.obs_kf[i] == small.obs_kf[a] and i != a][0]
        bad.obs_uv[a] = small.obs_uv[b]
    return bad


def test_check_reports_each_state_and_reads_only(gpu):
    from rsvio.ba import BundleBatch
    probs = _mixed() + [_swapped(_small())]
    gate = TT._gate()
    gates = [gate] * len(probs)
    gates[3] = TT._gate(TT.FIRST_STEREO, 0.1, 4.0, 1e-5)
    wins = _handles(probs)
    batch = BundleBatch(wins)

    def both():
        rep = batch.check_landmarks(gates)
        for i, w in enumerate(wins):
            info, n = w.check_landmarks(gates[i])
            assert rep[i][0].tobytes() == info.tobytes() and rep[i][1] == n, i
        return rep
    before = [w.state() for w in wins]
    rep = both()                                                 # before any run: the initial state
    TT._assert_info(rep[0][0], TT._np_landmarks(probs[0], gate, tri=False))
    TT._assert_info(rep[-1][0], TT._np_landmarks(probs[-1], gate, tri=False))
    assert all(np.array_equal(b[0], w.state()[0]) and np.array_equal(b[1], w.state()[1])
               for b, w in zip(before, wins))
    # the swapped landmark, triangulated behind the cameras through a wide gate: its slot only
    wide = [TT._gate(TT.FIRST_STEREO, -1e3, 1e3)] * len(probs)
    on = [i in (0, len(probs) - 1) for i in range(len(probs))]
    tri = batch.triangulate(None, wide, want=True, active=on)
    assert tri[-1][1]["flags"][7] == TT.OK and tri[-1][1]["max_depth"][7] < 0.0 and tri[1] is None
    rep = both()
    assert rep[-1][0]["flags"][7] == TT.DEPTH and rep[0][0]["flags"][7] == TT.OK
    assert int((rep[-1][0]["flags"] == TT.DEPTH).sum()) == 1 and rep[-1][1] == probs[-1].n_lm - 1
    res = batch.run()
    assert res[0].status > 0
    solved = [w.state() for w in wins]
    rep = both()                                                 # after a batch run: the solved state
    pose, pw = solved[0]
    TT._assert_info(rep[0][0], TT._np_landmarks(probs[0], gate, tri=False, pose7=pose, p_W=pw))
    assert all(a[0].tobytes() == w.state()[0].tobytes() and a[1].tobytes() == w.state()[1].tobytes()
               for a, w in zip(solved, wins))
    _close(batch, wins)


# ------------------------------------------------------------------------------------------
# 4: covariance, bits and references
# ------------------------------------------------------------------------------------------
def _cov_probs():
    return [TC._size_problem(*s) for s in SIZES] + [TC._pattern_problem("staircase")]


def test_covariance_slots_equal_the_single_call(gpu):
    from rsvio import ba as B
    probs = _cov_probs()
    wins = _handles(probs)
    batch = B.BundleBatch(wins)
    sel = [True, None, np.array([5, 0, 5, 17]), True, True, np.arange(0, 200, 7), True]

    def both(stage):
        got = batch.covariance(sel, full=True)
        assert batch.device_ms > 0.0
        for i, w in enumerate(wins):
            one = w.covariance(sel[i], full=True)
            assert one.status == B.COV_OK and _same_cov(got[i], one), (stage, i)
        return got
    c0 = both("initial")
    assert sorted({c.n_free for c in c0}) == [1, 2, 4, 9, 10, 11, 19]   # templates 1 .. 10, 13 and 20 in one call
    res = batch.run()
    assert all(r.status > 0 for r in res)
    c1 = both("after a batch run")
    assert not np.array_equal(c0[3].full, c1[3].full)
    for i in (1, 4, 6):                                          # a single run on some handles only
        assert wins[i].run(B.lm_cfg(max_iterations=2)).iterations >= 1
    c2 = both("after single runs on some")
    assert _same_cov(c1[0], c2[0]) and not np.array_equal(c1[4].full, c2[4].full)
    _close(batch, wins)


def test_covariance_slots_match_the_references(gpu, oracle):
    """One slot per template family against covariance_reference at test_covariance_gpu's CAP."""
    from rsvio.ba import BundleBatch
    probs = _cov_probs()
    wins = _handles(probs)
    batch = BundleBatch(wins)
    assert all(r.status > 0 for r in batch.run())
    got = batch.covariance(True, full=True)
    for i in (1, 4, 5, 6):                                       # 2, 10, 11 (padded to 13) and 19 (20) free keyframes
        TC._check(oracle, probs[i], wins[i], cov=got[i], what=f"batched slot {i}")
    _close(batch, wins)


# ------------------------------------------------------------------------------------------
# 5: singular slots beside healthy ones
# ------------------------------------------------------------------------------------------
def _edge_probs():
    healthy = TC._size_problem(3, 40)
    gauge = dataclasses.replace(healthy, kf_fixed=np.zeros(3, np.uint8))          # no fixed keyframe
    hub, _ = TC._huber_problem()
    behind = dataclasses.replace(hub, p_W=hub.p_W.copy())                         # test_cheirality_...'s window
    behind.p_W[0] = -behind.p_W[0] * 5.0
    return [healthy, gauge, TC._size_problem(5, 90), behind]


def _raw_cov_slots(probs, fill=-7.0):
    from rsvio import _lib
    slots = (_lib.BaCovSlot * len(probs))()
    bufs = []
    for s, p in zip(slots, probs):
        n = 6 * int((np.asarray(p.kf_fixed) == 0).sum())
        cc, cp = np.full((n, n), fill), np.full((p.n_kf, 36), fill)
        lm, fl = np.full((p.n_lm, 9), fill), np.full(p.n_lm, 9, np.uint8)
        s.cov_cc, s.cov_pose, s.cov_lm, s.lm_flags, s.n_sel = _lib.ptr(cc), _lib.ptr(cp), _lib.ptr(lm), _lib.ptr(fl), p.n_lm
        s.info.status = -77
        bufs.append((cc, cp, lm, fl))
    return slots, bufs


def test_covariance_singular_slots_leave_the_rest_alone(gpu):
    from rsvio import _lib
    from rsvio import ba as B
    probs = _edge_probs()
    wins, twins = _handles(probs), _handles(probs)
    batch, tbatch = B.BundleBatch(wins), B.BundleBatch(twins)
    slots, bufs = _raw_cov_slots(probs)
    before = [w.state() for w in wins]
    _lib.check(_lib.load().rsvio_ba_batch_covariance(batch._h, None, 2.0, slots, None))
    assert [s.info.status for s in slots] == [B.COV_OK, B.COV_CAMERA_SINGULAR, B.COV_OK, B.COV_LANDMARK_SINGULAR]
    assert (slots[1].info.n_singular, slots[1].info.n_free) == (0, 3)
    assert (slots[3].info.n_singular, slots[3].info.n_free) == (1, 2)
    for i in (1, 3):                                             # nothing written for a singular window
        cc, cp, lm, fl = bufs[i]
        assert (cc == -7.0).all() and (cp == -7.0).all() and (lm == -7.0).all() and (fl == 9).all()
    for i in (0, 2):                                             # the healthy slots: the single call's bits
        cc, cp, lm, fl = bufs[i]
        one = wins[i].covariance(landmarks=True, full=True)
        assert one.status == B.COV_OK and one.cost == slots[i].info.cost
        assert np.array_equal(cc, one.full) and np.array_equal(cp.reshape(-1, 6, 6), one.pose)
        assert np.array_equal(lm.reshape(-1, 3, 3), one.landmarks) and np.array_equal(fl, one.flags)
    # the state, and a following batch run, with and without the call
    for b, w in zip(before, wins):
        s = w.state()
        assert b[0].tobytes() == s[0].tobytes() and b[1].tobytes() == s[1].tobytes()
    res, tres = batch.run(), tbatch.run()
    for i in range(len(probs)):
        assert _same_result(res[i], tres[i]) and _same_state(wins[i], twins[i]), i
    assert res[0].status > 0 and res[2].status > 0
    _close(batch, tbatch, wins, twins)


# ------------------------------------------------------------------------------------------
# 6: subsets
# ------------------------------------------------------------------------------------------
def _raw_lm_slots(wins, want=True):
    from rsvio import _lib
    slots = (_lib.BaLandmarkSlot * len(wins))()
    bufs = []
    for s, w in zip(slots, wins):
        pw, info = np.full((max(w.n_lm, 1), 3), -7.0), np.zeros(max(w.n_lm, 1), _lib.LANDMARK_INFO_DTYPE)
        info["flags"] = -77
        s.n_lm, s.n_ok, s.status = w.n_lm, -77, -77
        if want:
            s.p_W_out, s.info_out = _lib.ptr(pw), _lib.ptr(info)
        bufs.append((pw, info))
    return slots, bufs


@pytest.mark.parametrize("on", [[1, 0, 0, 0], [0, 1, 1, 0], [0, 0, 0, 0]])
def test_subsets_leave_inactive_windows_untouched(gpu, on):
    """Window 3 holds no problem at all: accepted while inactive."""
    from rsvio import _lib
    from rsvio import ba as B
    lib = _lib.load()
    probs = [TC._size_problem(3, 40), _small(), TC._size_problem(5, 90)]
    wins = _handles(probs) + [B.BundleAdjuster(max_keyframes=4, max_landmarks=8, max_observations=64)]
    twins = _handles(probs)
    batch = B.BundleBatch(wins)
    act = (C.c_uint8 * 4)(*on)
    gate, cfg = TT._gate(TT.ALL_VIEWS), B.lm_cfg()
    ms = C.c_double(-1.0)
    # triangulate
    slots, bufs = _raw_lm_slots(wins)
    image = [bytes(s) for s in slots]
    _lib.check(lib.rsvio_ba_batch_triangulate(batch._h, act, C.byref(gate), slots, C.byref(ms)))
    for i in range(4):
        if on[i]:
            pw, info, n = twins[i].triangulate(gate=gate, want=True)
            assert np.array_equal(bufs[i][0], pw) and bufs[i][1].tobytes() == info.tobytes()
            assert (slots[i].n_ok, slots[i].status) == (n, 0)
        else:
            assert bytes(slots[i]) == image[i] and (bufs[i][0] == -7.0).all() and (bufs[i][1]["flags"] == -77).all()
    # run_active
    res = (_lib.BaResult * 4)()
    C.memset(res, 0x5a, C.sizeof(res))
    sentinel = bytes(res[0])
    _lib.check(lib.rsvio_ba_batch_run_active(batch._h, act, C.byref(cfg), res))
    for i in range(4):
        if on[i]:
            assert _same_result(res[i], twins[i].run()) and _same_state(wins[i], twins[i])
        else:
            assert bytes(res[i]) == sentinel
    # check
    slots, bufs = _raw_lm_slots(wins)
    image = [bytes(s) for s in slots]
    _lib.check(lib.rsvio_ba_batch_check_landmarks(batch._h, act, C.byref(gate), slots, C.byref(ms)))
    for i in range(4):
        if on[i]:
            info, n = twins[i].check_landmarks(gate)
            assert bufs[i][1].tobytes() == info.tobytes() and slots[i].n_ok == n
        else:
            assert bytes(slots[i]) == image[i] and (bufs[i][1]["flags"] == -77).all()
    # covariance
    cslots, cbufs = _raw_cov_slots(probs + [probs[0]])
    cslots[3].n_sel = 0
    image = [bytes(s) for s in cslots]
    _lib.check(lib.rsvio_ba_batch_covariance(batch._h, act, 2.0, cslots, C.byref(ms)))
    for i in range(4):
        if on[i]:
            one = twins[i].covariance(landmarks=True, full=True)
            assert cslots[i].info.status == B.COV_OK and np.array_equal(cbufs[i][0], one.full)
            assert np.array_equal(cbufs[i][2].reshape(-1, 3, 3), one.landmarks)
        else:
            assert bytes(cslots[i]) == image[i] and all((b == -7.0).all() for b in cbufs[i][:3])
    if not any(on):
        assert ms.value == 0.0
    # the Python methods: None for an inactive window
    assert [r is None for r in batch.check_landmarks(gate, active=on)] == [not a for a in on]
    assert [r is None for r in batch.covariance(active=on)] == [not a for a in on]
    assert [r is None for r in batch.run(active=on)] == [not a for a in on]
    _close(batch, wins, twins)


def test_run_active_null_is_batch_run_and_a_batch_of_one(gpu):
    from rsvio import _lib
    from rsvio import ba as B
    lib = _lib.load()
    probs = [TC._size_problem(3, 40), TC._size_problem(11, 200), TC._size_problem(12, 200)]
    wins, twins = _handles(probs), _handles(probs)
    batch, tbatch = B.BundleBatch(wins), B.BundleBatch(twins)
    cfg = B.lm_cfg()
    res = (_lib.BaResult * 3)()
    _lib.check(lib.rsvio_ba_batch_run_active(batch._h, None, C.byref(cfg), res))
    tres = tbatch.run()
    for i in range(3):
        assert _same_result(res[i], tres[i]) and res[i].status > 0 and _same_state(wins[i], twins[i])
    _close(batch, tbatch)
    # B = 1: every call on a batch of one window
    one, gate = B.BundleBatch(wins[:1]), TT._gate(TT.ALL_VIEWS)
    t = one.triangulate(gates=gate, want=True)[0]
    tt = twins[0].triangulate(gate=gate, want=True)
    assert np.array_equal(t[0], tt[0]) and t[1].tobytes() == tt[1].tobytes() and t[2] == tt[2]
    assert _same_result(one.run(active=[1])[0], twins[0].run()) and _same_state(wins[0], twins[0])
    assert one.check_landmarks(gate)[0][0].tobytes() == twins[0].check_landmarks(gate)[0].tobytes()
    assert _same_cov(one.covariance(True, full=True)[0], twins[0].covariance(True, full=True))
    _close(one, wins, twins)


# ------------------------------------------------------------------------------------------
# 7: refusals, each before any write
# ------------------------------------------------------------------------------------------
def test_refusals_come_before_any_write(gpu):
    from rsvio import _lib
    from rsvio import ba as B
    lib = _lib.load()
    probs = [TC._size_problem(3, 40), TC._size_problem(5, 90)]
    wins = _handles(probs)
    empty = B.BundleAdjuster(max_keyframes=4, max_landmarks=8, max_observations=64)
    gate, cfg = TT._gate(), B.lm_cfg()

    def refused(call, *words):
        assert call() == -1
        msg = lib.rsvio_last_error().decode()
        assert all(w in msg for w in words), msg

    def calls(batch, n, lm_slots, cov_slots, res):
        return [lambda: lib.rsvio_ba_batch_triangulate(batch._h, None, C.byref(gate), lm_slots, None),
                lambda: lib.rsvio_ba_batch_check_landmarks(batch._h, None, C.byref(gate), lm_slots, None),
                lambda: lib.rsvio_ba_batch_covariance(batch._h, None, 2.0, cov_slots, None),
                lambda: lib.rsvio_ba_batch_run_active(batch._h, (C.c_uint8 * n)(*([1] * n)), C.byref(cfg), res)]

    # an active window without a problem (slot 2)
    batch = B.BundleBatch(wins + [empty])
    lm_slots, lm_bufs = _raw_lm_slots(wins + [empty])
    cov_slots, cov_bufs = _raw_cov_slots(probs + [probs[0]])
    res = (_lib.BaResult * 3)()
    C.memset(res, 0x5a, C.sizeof(res))
    image = bytes(lm_slots), bytes(cov_slots), bytes(res)
    start = [w.state() for w in wins]
    for call in calls(batch, 3, lm_slots, cov_slots, res):
        refused(call, "problem", "2")
    # n_lm wrong in slot 1; lm_idx out of range in slot 1; huber_delta 0 and NaN
    ok = (C.c_uint8 * 3)(1, 1, 0)
    lm_slots[1].n_lm += 1
    image = bytes(lm_slots), image[1], image[2]
    refused(lambda: lib.rsvio_ba_batch_triangulate(batch._h, ok, C.byref(gate), lm_slots, None), "n_lm", "slot 1")
    refused(lambda: lib.rsvio_ba_batch_check_landmarks(batch._h, ok, C.byref(gate), lm_slots, None), "n_lm", "slot 1")
    idx = np.array([0, probs[1].n_lm], np.int32)
    cov_slots[1].lm_idx, cov_slots[1].n_sel = _lib.ptr(idx), 2
    image = image[0], bytes(cov_slots), image[2]
    refused(lambda: lib.rsvio_ba_batch_covariance(batch._h, ok, 2.0, cov_slots, None), "lm_idx", "slot 1")
    cov_slots[1].lm_idx, cov_slots[1].n_sel = None, probs[1].n_lm
    image = image[0], bytes(cov_slots), image[2]
    for delta in (0.0, -1.0, float("nan")):
        refused(lambda: lib.rsvio_ba_batch_covariance(batch._h, ok, delta, cov_slots, None), "huber_delta")
    # a bad gate in one slot, and no gate at all for a slot without its own
    lm_slots[1].n_lm -= 1
    bad_gate = TT._gate(TT.FIRST_STEREO, 5.0, 1.0)
    lm_slots[0].gate = C.pointer(bad_gate)
    image = bytes(lm_slots), image[1], image[2]
    refused(lambda: lib.rsvio_ba_batch_check_landmarks(batch._h, ok, C.byref(gate), lm_slots, None), "slot 0")
    refused(lambda: lib.rsvio_ba_batch_triangulate(batch._h, (C.c_uint8 * 3)(0, 1, 0), None, lm_slots, None), "slot 1")
    lm_slots[0].gate = None
    image = bytes(lm_slots), image[1], image[2]
    # a window with a solve in flight (slot 0)
    wins[0].run_async()
    for fn in (lambda: lib.rsvio_ba_batch_triangulate(batch._h, ok, C.byref(gate), lm_slots, None),
               lambda: lib.rsvio_ba_batch_check_landmarks(batch._h, ok, C.byref(gate), lm_slots, None),
               lambda: lib.rsvio_ba_batch_covariance(batch._h, ok, 2.0, cov_slots, None),
               lambda: lib.rsvio_ba_batch_run_active(batch._h, ok, C.byref(cfg), res)):
        refused(fn, "in flight", "0")
    assert wins[0].wait().status > 0
    # nothing was written by any refused call: slots, results, outputs, the other window's state
    assert (bytes(lm_slots), bytes(cov_slots), bytes(res)) == image
    assert all((b[0] == -7.0).all() and (b[1]["flags"] == -77).all() for b in lm_bufs)
    assert all((x == -7.0).all() for b in cov_bufs for x in b[:3])
    s = wins[1].state()
    assert s[0].tobytes() == start[1][0].tobytes() and s[1].tobytes() == start[1][1].tobytes()
    # and the same arguments, once valid, go through
    assert lib.rsvio_ba_batch_check_landmarks(batch._h, ok, C.byref(gate), lm_slots, None) == 0
    assert lm_slots[1].n_ok >= 0 and lm_slots[1].status == 0
    _close(batch, wins, empty)


# ------------------------------------------------------------------------------------------
# 8: WindowBatch against SlidingWindows on their own
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _other():
    from rsvio import synthetic as S
    p = S.ba_problem(n_kf=5, n_lm=90, kf_per_lm=3, seed=51, init_seed=52)
    return dataclasses.replace(p, p_W=TT._ray_start(p))


GATE_A = (TT.FIRST_STEREO, 0.1, 4.0)     # test_sliding_window_cull's: a bound of 4 m splits the depths
GATE_B = (TT.ALL_VIEWS, 0.1, 5.0)


def _three_windows():
    from rsvio.ba import SlidingWindow
    plain = SlidingWindow(4)
    for fr in TC._mirror_frames():
        plain.add_frame(fr)
    return [plain,
            TT._window(_small(), landmark_init="triangulate", gate=TT._gate(*GATE_A), cull=True),
            TT._window(_other(), landmark_init="triangulate", gate=TT._gate(*GATE_B), cull=True, covariance=True)]


def _ulp32(a, b):
    return np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b))))


def test_window_batch_mirrors_sliding_windows(gpu):
    from rsvio import synthetic as S
    from rsvio.ba import COV_LM_OK, COV_OK, WindowBatch
    mine, twins = _three_windows(), _three_windows()
    # the twins alone, and on the CPU: no cull decision of theirs sits on a threshold (_np_landmarks
    # asserts every depth away from the gate's bounds) and numpy keeps and culls the same landmarks
    built = [t.build_problem() for t in twins]
    assert [t.optimize() for t in twins] == [True, True, True]
    for t, b, g in ((twins[1], built[1], GATE_A), (twins[2], built[2], GATE_B)):
        pose7, fixed, p_init, lm, kf, cam, uv, tcb, ids = b
        prob = S.BAProblem(pose7, fixed, p_init, lm, kf, cam, uv, tcb, pose7, p_init)
        pose, pw = t.solver.last_state
        keep = TT._np_landmarks(prob, TT._gate(*g), tri=False, pose7=pose, p_W=pw)[2] == TT.OK
        assert 0 < keep.sum() < len(keep) and np.array_equal(t.map_ids, np.sort(ids[keep]))
    wb = WindowBatch(mine)
    assert wb.optimize() == [True, True, True]
    for i, (w, t) in enumerate(zip(mine, twins)):
        assert (w.last_result.status, w.last_result.iterations) == (t.last_result.status, t.last_result.iterations)
        assert w.last_triangulation == t.last_triangulation and w.fallbacks == t.fallbacks == 0, i
        assert np.array_equal(w.map_ids, t.map_ids) and w.map_version == t.map_version == 1
        assert w.map_pw.dtype == np.float32 and _ulp32(w.map_pw, t.map_pw), i
        assert all(np.abs(a.T_W_B - b.T_W_B).max() <= 1e-10 for a, b in zip(w.keyframes, t.keyframes)), i
    assert mine[1].last_triangulation[0] > 0 and mine[0].last_triangulation is None
    # the stored covariance: a single call made afterwards on the same handle, bit for bit
    w = mine[2]
    assert mine[0].pose_covariance is None and mine[1].pose_covariance is None
    cov = w.solver.covariance(landmarks=True)
    ids = built[2][8]
    seen = cov.flags == COV_LM_OK
    assert cov.status == COV_OK and np.array_equal(w.pose_covariance, cov.pose)
    assert sorted(w.landmark_covariance) == sorted(np.asarray(ids)[seen].tolist())
    for fid, c in zip(np.asarray(ids)[seen].tolist(), cov.landmarks[seen]):
        assert np.array_equal(w.landmark_covariance[fid], c)
    assert twins[2].pose_covariance is not None and twins[2].pose_covariance.shape == w.pose_covariance.shape
    # a second step with one window active: the others' maps stay as they were
    maps = [(w.map_ids.copy(), w.map_pw.copy()) for w in mine]
    assert wb.optimize(active=[False, True, False]) == [None, True, None]
    assert [w.map_version for w in mine] == [1, 2, 1]
    for i in (0, 2):
        assert np.array_equal(mine[i].map_ids, maps[i][0]) and np.array_equal(mine[i].map_pw, maps[i][1])
    # a window that is not full raises before anything is done
    mine[0].keyframes.popleft()
    with pytest.raises(RuntimeError, match="Need more keyframes"):
        wb.optimize()
    assert [w.map_version for w in mine] == [1, 2, 1]
    wb.close()
    for w in mine + twins:
        w.solver.close()
