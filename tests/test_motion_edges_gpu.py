"""B8 on the GPU at its edges: every input of the catalogue (oracle/pnp_cases.py) through
MotionTracker.track_motion against the oracle, under test_motion_gpu.py's contract -- integer
outcomes (status, iterations, observation count, keyframe flag) equal, T_W_B, the two norms and
both costs within 1e-9.  test_motion_reference_cpu.py shows on the same inputs that the oracle
agrees with an independent longdouble LM to 2e-13 and that no decision of any case is within 10 %
of its threshold, so an unequal integer outcome here is a wrong branch on the device, not rounding.

What the catalogue reaches that test_motion_gpu.py does not: the hash join's probe loop past the
first bucket, its wrap-around, a miss by a free slot at depth 9 and by exhausting the run, keys
that differ in one 32-bit word only, the id 2^64 - 1 in and out of the map, four maps in a row on
one handle; se3_plus_r's sincos branch (steps of 0.3 to 1.34 rad), rejected steps, and the exits
LM_PARAM_TOL, LM_MAX_ITERS, LM_NUMFAIL and LM_LINSOLVE; a last keyframe whose R_B_W has a
negative trace; and the join loop's stride edges up to the LDS cap of 4,096 features, run back to
back on one handle in both orders.  LM_TRUST_REGION stays uncovered (oracle/pnp_cases.py).

Largest GPU-vs-oracle deviations observed on an MI355X, per group (max |dT_W_B| / cost relative
to max(1, cost) / the two norms), against the bound of 1e-9:
  LM branches (big rotations, tolerances, limits)  1.1e-15 / 2.8e-15 / 7.2e-16
  one to three features (rank-deficient up to lambda)  2.9e-13 / 4.2e-18 / 1.5e-14
  poses with trace(R_B_W) < 0                      3.3e-16 / 9.7e-17 / 2.2e-16
  feature counts                                   1.3e-13 (n1+1; 5.8e-16 from 64 features up) / 2.8e-15 / 2.8e-14
  join cases and maps in a row                     8.3e-16 / 2.8e-17 / 7.0e-16
No case needs a bound of its own, and no case showed a kernel or host-table bug.
"""
import numpy as np
import pytest

from oracle import pnp_cases as PC

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9

LM_POSE = [("lm", n) for n in PC.LM_CASES] + [("pose", n) for n in PC.POSE_CASES]
COUNT_NAMES = [n for n in PC.COUNT_CASES if n != "duplicate-id"]


def _oracle(oracle, c):
    return oracle.track_motion(*c.args(), cfg=oracle.lm_cfg(**{"max_iterations": 10, **c.cfg}))


def _run(mt, c, set_map=True):
    from rsvio.motion import pnp_cfg
    if set_map:
        mt.set_map(c.map_ids, c.map_pw)
    return mt.track_motion(c.ids_l, c.uv_l, c.ids_r, c.uv_r, c.T_last, c.T_C_B2, cfg=pnp_cfg(**c.cfg))


def _ints(r):
    return (r.status, r.iterations, r.n_observations, int(r.is_keyframe))


def _bits(r):
    """Everything the launch computed (not its duration), for bitwise comparison."""
    return (_ints(r), r.T_W_B.tobytes(), np.array([r.initial_cost, r.final_cost, r.translation_norm,
                                                   r.rotation_norm]).tobytes())


def _check(r, o, tag, nonfinite=False):
    To = np.array(o.T_W_B[:]).reshape(4, 4)
    dT = float(np.abs(r.T_W_B - To).max())
    dc = [abs(a - b) / max(1.0, abs(b)) for a, b in ((r.initial_cost, o.initial_cost), (r.final_cost, o.final_cost))]
    dn = [abs(r.translation_norm - o.translation_norm), abs(r.rotation_norm - o.rotation_norm)]
    print(f"DEV {tag}: gpu {_ints(r)} oracle {_ints(o)} dT {dT:.2e} dcost {dc[0]:.2e} {dc[1]:.2e} "
          f"dnorm {dn[0]:.2e} {dn[1]:.2e} cost {o.initial_cost:.6g} -> {o.final_cost:.6g} "
          f"(gpu {r.initial_cost:.6g} -> {r.final_cost:.6g})")
    assert _ints(r) == _ints(o)
    assert dT <= POSE_TOL
    if nonfinite:
        for v in (r.initial_cost, r.final_cost, o.initial_cost, o.final_cost):
            assert not np.isfinite(v)
    else:
        assert dc[0] <= 1e-9 and dc[1] <= 1e-9
    assert dn[0] <= 1e-9 and dn[1] <= 1e-9
    if r.status <= 0:
        assert r.is_keyframe and np.array_equal(r.T_W_B, np.eye(4))
    assert 0.0 < r.kernel_ms < 100.0


@pytest.fixture(scope="module")
def motion(gpu):
    from rsvio.motion import MotionTracker
    mt = MotionTracker()
    yield mt
    mt.close()


@pytest.mark.parametrize("group,name", LM_POSE, ids=["-".join(c) for c in LM_POSE])
def test_lm_branches_and_poses(motion, oracle, group, name):
    c = PC.get(group, name)
    r = _run(motion, c)
    o = _oracle(oracle, c)
    _check(r, o, f"{group} {name}", nonfinite=c.nonfinite)
    if c.expect is not None:
        assert (r.status, r.iterations) == c.expect
    if c.n_obs is not None:
        assert r.n_observations == c.n_obs
    if c.same_as:
        # the poisoned coordinate belongs to a feature without a map point: the device's result
        # is its own clean-frame result, bit for bit
        assert _bits(r) == _bits(_run(motion, PC.get(group, c.same_as), set_map=False))


def test_big_rotation_twice_is_bit_identical(motion):
    """Fixed-order reductions: the ten-iteration, six-reject run repeats exactly."""
    c = PC.get("lm", "big-rot-A")
    a = _run(motion, c)
    b = _run(motion, c, set_map=False)
    assert a.status == 3 and _bits(a) == _bits(b)


@pytest.fixture(scope="module")
def count_sweep(gpu):
    """The slices of one frame on ONE handle, back to back, in the catalogue's order and then in
    reverse: a value left in LDS or in the control state by a larger frame would show in the next
    smaller one."""
    from rsvio.motion import MotionTracker
    mt = MotionTracker()
    try:
        first = PC.get("count", COUNT_NAMES[0])
        mt.set_map(first.map_ids, first.map_pw)
        out = {}
        for order, names in (("fwd", COUNT_NAMES), ("rev", COUNT_NAMES[::-1])):
            for n in names:
                out[order, n] = _run(mt, PC.get("count", n), set_map=False)
        return out
    finally:
        mt.close()


@pytest.mark.parametrize("name", COUNT_NAMES)
def test_feature_counts(count_sweep, oracle, name):
    c = PC.get("count", name)
    o = _oracle(oracle, c)
    assert o.n_observations == c.n_obs
    for order in ("fwd", "rev"):
        r = count_sweep[order, name]
        _check(r, o, f"count {name} {order}")
        assert r.n_observations == c.n_obs
    assert _bits(count_sweep["fwd", name]) == _bits(count_sweep["rev", name])


def test_duplicate_feature_id_counts_twice(motion, oracle):
    c = PC.get("count", "duplicate-id")
    r = _run(motion, c)
    _check(r, _oracle(oracle, c), "count duplicate-id")
    assert r.n_observations == c.n_obs


@pytest.mark.parametrize("name", list(PC.JOIN_CASES))
def test_join_cases(motion, oracle, name):
    c = PC.get("join", name)
    motion.set_map(c.map_ids, c.map_pw)
    stats = motion.map_stats()
    assert {k: stats[k] for k in c.stats} == c.stats
    r = _run(motion, c, set_map=False)
    _check(r, _oracle(oracle, c), f"join {name}")
    assert r.n_observations == c.n_obs


def test_maps_in_a_row_on_one_handle(gpu, oracle):
    """set_map(9,000), (40), (0), (9,000) on one handle; the frame run after each has features
    whose ids were in the previous map only.  Nothing of a former table may answer."""
    from rsvio.motion import MotionTracker
    m, maps = PC.remap_sequence()
    mt = MotionTracker()
    try:
        n_obs = []
        for label, ids, pw in maps:
            mt.set_map(ids, pw)
            s = mt.map_stats()
            assert (s["n_map"], s["has_top"]) == (len(ids), 0)
            assert s["buckets"] == {9000: 16384, 40: 64, 0: 16}[len(ids)]
            r = mt.track_motion(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2)
            o = oracle.track_motion(m.ids_l, m.uv_l, m.ids_r, m.uv_r, ids, pw, m.T_W_B_last_kf, m.T_C_B2)
            _check(r, o, f"remap {label}")
            n_obs.append(r.n_observations)
        assert n_obs[0] == n_obs[3] > 1500 and n_obs[1] == 80 and n_obs[2] == 0
    finally:
        mt.close()
