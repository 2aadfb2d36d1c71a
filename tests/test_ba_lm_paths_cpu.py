"""What the CPU oracle does on the windows of test_ba_lm_paths_gpu.py, from oracle.ba_solve_trace
alone -- so that none of the GPU tests can pass on a trivial or a knife-edge case.

Every existing BA window accepts every LM step until the cost tolerance ends the solve.  The
windows here (rsvio.synthetic.ba_lm_window) do not; CASES pins, per window and configuration, the
oracle's status, iteration count and accept pattern ('A' accepted, 'R' rejected, one letter per
iteration that reached a decision: an iteration that ends the solve on a tolerance has none).  The
GPU file imports CASES.

The margins asserted here are conditions, not measurements: with |rho| >= 0.1 on every decision,
and every relative cost change and step ratio outside a factor 1.5 of its tolerance, no decision
of these solves depends on the order in which a cost or a dot product was summed, so the device
(tree order) and the oracle (sequential) must take the same path.

Seeds: W3 and W5 are not the windows first tried for them.  ba_problem(n_kf=12, n_lm=192,
kf_per_lm=4, seed=52, init_seed=53, ...) ends with a relative cost change of 8.4e-7 against the
tolerance 1e-6 (a factor 1.19), and seed=43, init_seed=44 at the larger noise has 1.17e-6 at its
third iteration (1.17); both fail the factor-1.5 condition.  W3 is seed=126, init_seed=127 (the
same pattern, AAARR...), W5 seed=58, init_seed=59: the first seeds of a scan upwards whose
pattern has two consecutive cheirality rejects after accepted steps and which meet every margin.
"""
import numpy as np
import pytest

COST_TOL, PARAM_TOL = 1e-6, 1e-9   # lm_cfg's defaults (sliding_window.rs:132-133)

# name: (window, configuration, status, iterations, pattern)
CASES = {
    "W1": ("W1", dict(max_iterations=30), 1, 9, "AARAAAAA"),
    "W1_max3": ("W1", dict(max_iterations=3), 3, 3, "AAR"),            # status 3 on a rejected step
    "W1_chol": ("W1", dict(max_iterations=30, linear_solver=1), 1, 9, "AARAAAAA"),
    "W2_d2": ("W2", dict(huber_delta=2.0, max_iterations=12), 3, 12, "RRAARAAAAAAA"),
    "W2_d005": ("W2", dict(huber_delta=0.05, max_iterations=8), 3, 8, "AAAAAAAA"),
    "W3": ("W3", dict(), 1, 12, "AAARRAAAAAA"),
    "W3b": ("W3b", dict(), 1, 10, "AARAAAAAA"),
    "W4": ("default5", dict(parameter_tolerance=1e-3, cost_tolerance=1e-12), 2, 5, "AAAA"),
    "W5": ("W5", dict(max_iterations=30), 1, 14, "AAARRAAAAAAAA"),
    # the batches' configuration (max_iterations=30 for every member)
    "default5_30": ("default5", dict(max_iterations=30), 1, 6, "AAAAA"),
    "default4_30": ("default4", dict(max_iterations=30), 1, 6, "AAAAA"),
    "W2_d2_30": ("W2", dict(huber_delta=2.0, max_iterations=30), 3, 30, "RRAARAAAAAAAAAAAAAAAAAAAAARRRA"),
    "W3_30": ("W3", dict(max_iterations=30), 1, 12, "AAARRAAAAAA"),
}
N_OBS = {"W1": 768, "W2": 768, "default5": 768, "default4": 768, "W3": 1536, "W3b": 1536, "W5": 1536}

_windows = {}


def window(name):
    """The named window, generated once; never modified by a test."""
    if name not in _windows:
        from rsvio import synthetic as S
        _windows[name] = S.ba_lm_window(name)
    return _windows[name]


def pattern(res, trace):
    """One letter per iteration that reached the accept / reject decision."""
    rows = trace if res.status == 3 else trace[:-1]   # statuses 1 and 2 end inside their last iteration
    return "".join("A" if t["accepted"] else "R" for t in rows)


@pytest.fixture(scope="module")
def traces(oracle):
    """Per case: (pose, points, result, trace) of the sequential oracle."""
    oracle.set_ba_threads(1)
    return {k: oracle.ba_solve_trace(window(w), oracle.lm_cfg(**cfg)) for k, (w, cfg, *_) in CASES.items()}


def test_trace_leaves_the_solve_bit_identical(oracle, traces):
    """ba_solve and ba_solve_trace share one loop: the same bits on config 3 and on W1."""
    from rsvio import synthetic as S
    for prob, cfg in ((S.ba_problem(), {}), (window("W1"), CASES["W1"][1])):
        po, pwo, ro = oracle.ba_solve(prob, oracle.lm_cfg(**cfg))
        pt, pwt, rt, tr = oracle.ba_solve_trace(prob, oracle.lm_cfg(**cfg))
        assert (ro.status, ro.iterations, ro.initial_cost, ro.final_cost) == \
               (rt.status, rt.iterations, rt.initial_cost, rt.final_cost)
        assert np.array_equal(po, pt) and np.array_equal(pwo, pwt)
        assert len(tr) == ro.iterations and tr[0]["cost"] == ro.initial_cost
        assert tr[0]["lam"] == 1e-4 and tr[0]["nu"] == 2.0


@pytest.mark.parametrize("name", list(CASES))
def test_status_iterations_pattern(traces, name):
    win, _, status, iters, pat = CASES[name]
    _, _, res, tr = traces[name]
    assert window(win).n_obs == N_OBS[win]
    assert (res.status, res.iterations, pattern(res, tr)) == (status, iters, pat)
    # lambda and nu follow the rule: nu doubles over consecutive rejects and resets on an accept
    for a, b in zip(tr, tr[1:]):
        if a["accepted"]:
            f = 2.0 * a["rho"] - 1.0
            assert b["nu"] == 2.0 and b["lam"] == a["lam"] * max(1.0 / 3.0, 1.0 - f * f * f)
            assert b["cost"] == a["new_cost"]
        else:
            assert b["nu"] == 2.0 * a["nu"] and b["lam"] == a["lam"] * a["nu"] and b["cost"] == a["cost"]


def test_coverage():
    pats = {k: (c[2], c[4]) for k, c in CASES.items()}
    every = [p for _, p in pats.values()]
    assert any("AR" in p for p in every)                 # a reject that follows an accept
    assert any("RR" in p for p in every)                 # two consecutive rejects (nu reaches 4)
    assert any("RRR" in p for p in every)                # and three (nu reaches 8)
    assert any("RA" in p for p in every)                 # an accept that follows a reject
    assert pats["W1"][1][2] == "R"                       # a reject as iteration 3: a new handle's first chunk
    assert {1, 2, 3} <= {s for s, _ in pats.values()}
    assert any(s == 3 and p[-1] == "A" for s, p in pats.values())
    assert any(s == 3 and p[-1] == "R" for s, p in pats.values())
    assert any("R" in pats[k][1] for k in ("W3", "W3b", "W5"))   # past 10 free keyframes
    assert all(window(k).n_kf == 12 for k in ("W3", "W3b", "W5"))


@pytest.mark.parametrize("name", list(CASES))
def test_margins(traces, name):
    """No decision of the case is near its threshold."""
    cfg = CASES[name][1]
    ct, pt = cfg.get("cost_tolerance", COST_TOL), cfg.get("parameter_tolerance", PARAM_TOL)
    _, _, res, tr = traces[name]
    for i, t in enumerate(tr):
        assert not (pt / 1.5 < t["step_ratio"] < pt * 1.5), (i, t)
        if np.isnan(t["rho"]):                            # ended on the parameter tolerance
            assert res.status == 2 and i == len(tr) - 1
            continue
        assert abs(t["rho"]) >= 0.1, (i, t)
        assert not (ct / 1.5 < t["rel_dcost"] < ct * 1.5), (i, t)


@pytest.mark.parametrize("name", list(CASES))
def test_reference_is_insensitive_to_summation_order(oracle, traces, name):
    """The oracle at 5 threads (5 landmark ranges summed in range order) against the sequential
    one: the same path, poses within 1e-9 and points within 1e-8 -- two orders inside the GPU
    file's tolerances.

    One case is given 1e-7 on its points, one order inside: W2 at delta 2.0 under the batches'
    max_iterations=30.  With a tenth of its observations gross outliers at full weight the window
    keeps sliding along a weakly constrained direction (steps of 0.2 to 0.45 of |x| per iteration
    while the cost moves by 1e-3 to 1e-5 of itself), and rounding differences grow along it: the
    two orders differ by 2e-11 after the table's 12 iterations and by 6.8e-8 after 30, with the
    same 30 decisions.  That is the reference's own spread on this case, not a bound chosen from
    any device result; the GPU tolerance of 1e-6 stays 15 times outside it."""
    win, cfg, *_ = CASES[name]
    p1, w1, r1, t1 = traces[name]
    try:
        oracle.set_ba_threads(5)
        p5, w5, r5, t5 = oracle.ba_solve_trace(window(win), oracle.lm_cfg(**cfg))
    finally:
        oracle.set_ba_threads(1)
    assert (r1.status, r1.iterations, pattern(r1, t1)) == (r5.status, r5.iterations, pattern(r5, t5))
    dp, dw = np.abs(p1 - p5).max(), np.abs(w1 - w5).max()
    print(f"{name}: 1 vs 5 threads: poses {dp:.1e}, points {dw:.1e}")
    assert dp <= 1e-9 and dw <= (1e-7 if name == "W2_d2_30" else 1e-8)


# the cases whose reduced system at a rejected prefix the GPU file compares at the oracle's own
# state (S, b within 1e-9 of their maxima, cost within 1e-10)
SYSTEM_AT_ORACLE_STATE = ("W1", "W2_d2", "W3")


@pytest.mark.parametrize("name", SYSTEM_AT_ORACLE_STATE + ("W5",))
def test_reference_system_at_rejected_prefixes(oracle, name):
    """How far the oracle's own two summation orders are apart in the reduced system at the state
    a prefix ending on a rejected step returns.  For SYSTEM_AT_ORACLE_STATE it is at least one
    order inside the GPU file's bounds, so that comparison tests the device.  For W5 it is not:
    one weakly observed landmark leaves the two states 8.8e-9 apart after the third step, and
    the systems there 7.6e-11 (S), 4.8e-10 (b) and 3.6e-10 (cost) apart -- the last beyond the
    1e-10 bound -- so the GPU file compares W5's system at one common state only."""
    import dataclasses
    win, cfg, _, _, pat = CASES[name]
    prob, delta = window(win), cfg.get("huber_delta", 2.0)
    worst = np.zeros(3)
    for k in [i + 1 for i, c in enumerate(pat) if c == "R"]:
        sys_ = []
        for threads in (1, 5):
            try:
                oracle.set_ba_threads(threads)
                po, pwo, _ = oracle.ba_solve(prob, oracle.lm_cfg(**{**cfg, "max_iterations": k}))
            finally:
                oracle.set_ba_threads(1)
            sys_.append(oracle.ba_build_system(dataclasses.replace(prob, pose7=po, p_W=pwo), 1e-4, delta))
        (S1, b1, c1), (S5, b5, c5) = sys_
        worst = np.maximum(worst, [np.abs(S1 - S5).max() / np.abs(S1).max(), np.abs(b1 - b5).max() / np.abs(b1).max(),
                                   abs(c1 - c5) / c1])
    print(f"{name}: 1 vs 5 threads at rejected prefixes: S {worst[0]:.1e}  b {worst[1]:.1e}  cost {worst[2]:.1e}")
    if name in SYSTEM_AT_ORACLE_STATE:
        assert worst[0] <= 1e-10 and worst[1] <= 1e-10 and worst[2] <= 1e-11
    else:
        assert worst[2] > 1e-10


def huber_engaged(oracle, prob, delta):
    """Fraction of the residuals whose Huber weight is below 1 at the initial state (|r|^2 > delta^2,
    the oracle's and se3.hpp's rule; a residual behind the camera is the 1e6 penalty)."""
    n = 0
    for i in range(prob.n_obs):
        k, cam = prob.obs_kf[i], prob.obs_cam[i]
        r, _ = oracle.factor_linearize(prob.p_W[prob.obs_lm[i]], prob.pose7[k], prob.T_C_B2[cam], prob.obs_uv[i])
        n += bool(r[0] * r[0] + r[1] * r[1] > delta * delta)
    return n / prob.n_obs


def test_huber_engagement(oracle):
    frac = huber_engaged(oracle, window("W2"), 0.05)
    print(f"W2 at delta 0.05: {100 * frac:.1f} % of the residuals down-weighted")
    assert 0.05 < frac < 0.95
    assert huber_engaged(oracle, window("default5"), 2.0) == 0.0
