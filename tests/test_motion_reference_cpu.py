"""The catalogue of track_motion edge inputs (oracle/pnp_cases.py) on the CPU: the oracle against
an independent numpy longdouble LM on rotation matrices (oracle/pnp_reference.py), and the
QUALIFICATION that makes the device test on the same inputs (test_motion_edges_gpu.py) meaningful:
no decision of any case hangs on rounding.  At every iteration of every case, in the reference's
log, the cost-tolerance and parameter-tolerance ratios lie outside [0.9, 1.1], |gain ratio| is at
least 1e-3, and the keyframe norms are 1e-3 away from their thresholds.  A case that stops
qualifying gets another seed, not an exemption.

Oracle vs reference: status, iterations and observation count equal, T_W_B within 1e-11, costs
within 1e-11 relative (observed: <= 2e-13, the largest on the one- and two-feature frames, whose
system is rank-deficient up to lambda).  A cost is a sum of squared differences of O(1) numbers, so
in f64 it carries an absolute error of about |r| eps = sqrt(2 cost) eps whatever its size; the
bound allows 16 of those beside the relative term (it matters only on the single-observation
frame, whose final cost of 7e-20 is below the f64 resolution of its own residual).

The join cases are checked against a Python restatement of the host hash table: each is built to
a run length, a wrap-around and a kind of miss, and says so; the device test compares the same
numbers with MotionTracker.map_stats().
"""
import math

import numpy as np
import pytest

from oracle import pnp_cases as PC
from oracle import pnp_reference as PR

T_TOL = 1e-11
COST_RTOL = 1e-11
EPS = 2.0 ** -52

REF_CASES = [("lm", n) for n in PC.LM_CASES] + [("pose", n) for n in PC.POSE_CASES]
_ids = lambda cases: ["-".join(c) for c in cases]  # noqa: E731

_cache = {}


def _both(oracle, group, name):
    """(case, oracle result, reference result), computed once per case."""
    if (group, name) not in _cache:
        c = PC.get(group, name)
        o = oracle.track_motion(*c.args(), cfg=oracle.lm_cfg(**{"max_iterations": 10, **c.cfg}))
        _cache[group, name] = (c, o, PR.track_motion_ref(*c.args(), cfg=c.cfg))
    return _cache[group, name]


def _cost_close(a, b):
    return abs(a - b) <= COST_RTOL * abs(b) + 16 * EPS * math.sqrt(2 * abs(b))


@pytest.mark.parametrize("group,name", REF_CASES, ids=_ids(REF_CASES))
def test_oracle_matches_longdouble_reference(oracle, group, name):
    c, o, r = _both(oracle, group, name)
    To = np.array(o.T_W_B[:]).reshape(4, 4)
    print(f"{name}: oracle {(o.status, o.iterations, o.n_observations)} ref {(r.status, r.iterations)} "
          f"dT {float(np.abs(r.T_W_B - To).max()):.2e} cost {o.initial_cost:.6g} -> {o.final_cost:.6g} "
          f"(ref {r.initial_cost:.6g} -> {r.final_cost:.6g})")
    assert (o.status, o.iterations, o.n_observations) == (r.status, r.iterations, r.n_observations)
    if c.expect is not None:
        assert (o.status, o.iterations) == c.expect
    if c.n_obs is not None:
        assert o.n_observations == c.n_obs
    assert float(np.abs(r.T_W_B - To).max()) <= T_TOL
    if c.nonfinite:
        assert not math.isfinite(o.initial_cost) and not math.isfinite(o.final_cost)
        assert not math.isfinite(r.initial_cost) and not math.isfinite(r.final_cost)
    else:
        assert _cost_close(r.initial_cost, o.initial_cost) and _cost_close(r.final_cost, o.final_cost)
    if o.status <= 0:
        assert o.is_keyframe == 1 and np.array_equal(To, np.eye(4))


@pytest.mark.parametrize("group,name", REF_CASES, ids=_ids(REF_CASES))
def test_no_decision_hangs_on_rounding(oracle, group, name):
    _, o, r = _both(oracle, group, name)
    for k, e in enumerate(r.log):
        assert e.param_ratio < 0.9 or e.param_ratio > 1.1, (k, e)
        if e.cost_ratio is not None:
            assert e.cost_ratio < 0.9 or e.cost_ratio > 1.1, (k, e)
            assert abs(e.rho) >= 1e-3, (k, e)
    if o.status > 0:
        assert abs(o.translation_norm - 0.05) > 1e-3 and abs(o.rotation_norm - 0.05) > 1e-3


def test_cases_reach_the_branches_they_exist_for(oracle):
    log = lambda n: _both(oracle, "lm", n)[2].log  # noqa: E731
    for name in ("big-rot-A", "big-rot-B", "big-rot-C"):
        acc = [e.accepted for e in log(name)]
        assert any(a is False and b is True for a, b in zip(acc, acc[1:])), name   # a reject, then an accept
    assert sum(e.accepted is False for e in log("big-rot-A")) == 6
    assert sum(e.accepted is False for e in log("big-rot-B")) == 9
    # the step rotation is past se3_plus_r's switch to sincos at |w| = 1/4 -- on an ACCEPTED step
    for name in ("big-rot-A", "big-rot-C", "sincos-only"):
        assert any(e.accepted and e.angle > 0.25 for e in log(name)), name
    assert max(e.angle for e in log("big-rot-C")) > 1.3
    assert log("sincos-only")[0].angle > 0.3 and all(e.accepted is not False for e in log("sincos-only"))
    # every exit but LM_TRUST_REGION (see oracle/pnp_cases.py) and LM_SKIPPED (test_motion_cpu.py)
    reached = {_both(oracle, "lm", n)[1].status for n in PC.LM_CASES}
    assert reached == {PR.LM_COST_TOL, PR.LM_PARAM_TOL, PR.LM_MAX_ITERS, PR.LM_NUMFAIL, PR.LM_LINSOLVE}
    for name in ("param-tol-0", "max-iter-0"):
        o = _both(oracle, "lm", name)[1]
        assert o.final_cost == o.initial_cost
    # an unmatched feature's coordinates never enter: the result is the clean frame's, bit for bit
    clean = _both(oracle, "lm", "clean")[1]
    for name in ("nan-unmatched", "inf-unmatched"):
        o = _both(oracle, "lm", name)[1]
        assert bytes(o) == bytes(clean)


@pytest.mark.parametrize("name", list(PC.POSE_CASES))
def test_pose_cases_have_negative_trace(oracle, name):
    c, o, _ = _both(oracle, "pose", name)
    assert np.trace(c.T_last[:3, :3]) < 0.0 and c.facts["trace"] < 0.0
    # a rigid motion of the world changes nothing but the f32 rounding of the map points
    clean = _both(oracle, "lm", "clean")[1]
    assert (o.status, o.iterations, o.n_observations) == (clean.status, clean.iterations, clean.n_observations)
    assert abs(o.final_cost - clean.final_cost) < 1e-6 * clean.final_cost


@pytest.mark.parametrize("name", list(PC.COUNT_CASES))
def test_count_cases(oracle, name):
    c = PC.get("count", name)
    o = oracle.track_motion(*c.args())
    assert o.n_observations == c.n_obs
    assert len(c.ids_l) + len(c.ids_r) <= 4096
    if c.n_obs >= 64:
        assert (o.status, o.iterations) == (1, 3)
    if name == "duplicate-id":
        ids, n = np.unique(c.ids_l, return_counts=True)
        assert n.max() == 2 and np.isin(ids[n == 2], c.map_ids).all()
        assert c.n_obs == np.isin(c.ids_l, c.map_ids).sum() + np.isin(c.ids_r, c.map_ids).sum()


def test_hash_restatement():
    assert [PR.table_buckets(n) for n in (0, 1, 16, 17, 40, 64, 65, 9000)] == [16, 16, 16, 32, 64, 64, 128, 16384]
    ids = np.array([1, 2, 12345678901234567, PR.TOP_ID - 1, 1 << 63], np.uint64)
    for mask in (15, 63, 16383):
        assert PR.map_bucket_array(ids, mask).tolist() == [PR.map_bucket(i, mask) for i in ids.tolist()]
    assert PR.map_bucket(1, 0xFFFFFF) == 0x9E3779B97F4A7C15 >> 40


@pytest.mark.parametrize("name", list(PC.JOIN_CASES))
def test_join_cases_hit_what_they_aim_at(oracle, name):
    c = PC.get("join", name)
    table = PR.build_table(c.map_ids)
    for k, v in c.stats.items():
        assert table[k] == v, k
    feats = np.concatenate([c.ids_l, c.ids_r])
    ends = {int(i): PR.lookup_depth(i, table, c.map_ids) for i in np.unique(feats)}
    hits = {i for i, e in ends.items() if e[0] == "hit"}
    assert hits == set(c.map_ids.tolist()) & set(feats.tolist())
    o = oracle.track_motion(*c.args())
    assert o.n_observations == c.n_obs == sum(int(i) in hits for i in feats.tolist())
    assert (o.status, o.iterations) == (1, 3)
    if c.same_as:
        assert bytes(o) == bytes(oracle.track_motion(*PC.get("join", c.same_as).args()))
    if name.startswith("collide"):
        n = len(c.map_ids)
        assert all(PR.map_bucket(i, 63) == 63 for i in c.map_ids.tolist())
        assert sorted(table["depth"].values()) == sorted(k // 4 for k in range(n))      # 63 -> 0 -> ... -> 8
        assert hits == set(c.map_ids.tolist())                                         # a hit at every depth
        assert table["fill"][63] == 4 and table["fill"][8] == n - 36 and sum(table["fill"]) == n
        end = ("exhausted", 9) if n == 40 else ("free", 9)
        assert c.facts["miss_run_end"] == end[0]
        assert len(c.facts["miss_run"]) >= 12 and all(ends[i] == end for i in c.facts["miss_run"])
        assert len(c.facts["miss_empty"]) >= 12 and all(ends[i] == ("free", 0) for i in c.facts["miss_empty"])
    if name == "word-halves":
        (a0, a1), (b0, b1) = c.facts["same_low"], c.facts["same_high"]
        assert a0 & 0xFFFFFFFF == a1 & 0xFFFFFFFF and a0 >> 32 != a1 >> 32
        assert b0 >> 32 == b1 >> 32 and b0 & 0xFFFFFFFF != b1 & 0xFFFFFFFF
        assert PR.map_bucket(a0, 63) == PR.map_bucket(a1, 63) and PR.map_bucket(b0, 63) == PR.map_bucket(b1, 63)
        for inmap, only_feature in ((a0, a1), (b0, b1)):
            assert inmap in hits and ends[only_feature][0] == "free"
            assert only_feature in feats.tolist() and only_feature not in c.map_ids.tolist()
        assert min(c.map_ids.min(), feats.min()) >= 1 << 32
    if name == "top-id":
        assert c.map_ids[-1] == PR.TOP_ID and PR.TOP_ID in hits
    if name == "top-id-features-only":
        assert PR.TOP_ID in feats.tolist() and PR.TOP_ID not in hits


def test_remap_sequence(oracle):
    m, maps = PC.remap_sequence()
    n_obs = [oracle.track_motion(m.ids_l, m.uv_l, m.ids_r, m.uv_r, ids, pw, m.T_W_B_last_kf, m.T_C_B2).n_observations
             for _, ids, pw in maps]
    assert [len(ids) for _, ids, _ in maps] == [9000, 40, 0, 9000]
    assert n_obs[0] == n_obs[3] > 1500 and n_obs[1] == 80 and n_obs[2] == 0
    assert [PR.table_buckets(len(ids)) for _, ids, _ in maps] == [16384, 64, 16, 16384]
