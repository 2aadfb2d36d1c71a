"""The LM loop of the BA solve (ba.hip: K4 / K4c / K5 / K6 / K7, lm_update, lm_decide) on windows
that reject steps, against the f64 CPU oracle.

Every other BA window of the suite accepts every step until the cost tolerance ends the solve.
The windows here (rsvio.synthetic.ba_lm_window) reject steps, end on the parameter tolerance or
run with Huber weights below 1; test_ba_lm_paths_cpu.py pins what the oracle does on each
(CASES: status, iterations, accept pattern) and proves from the oracle alone that no decision of
theirs is near a threshold, so the device must take the same path:

    W1       5 KF, 768 obs    max_iterations=30        status 1,  9 it   AARAAAAA
    W2       5 KF, 768 obs    delta 2.0,  max 12       status 3, 12 it   RRAARAAAAAAA
    W2                        delta 0.05, max 8        status 3,  8 it   AAAAAAAA   (Huber engaged)
    W3      12 KF, 1536 obs   default                  status 1, 12 it   AAARRAAAAAA
    W3b     12 KF, 1536 obs   default                  status 1, 10 it   AARAAAAAA
    W4       5 KF, 768 obs    parameter_tolerance 1e-3 status 2,  5 it   AAAA
    W5      12 KF, 1536 obs   max_iterations=30        status 1, 14 it   AAARRAAAAAAAA (cheirality)

What is checked: the prefix sweep (max_iterations = 1..K on fresh handles: the device's accept
pattern, every intermediate state, and that a rejected step returns the pre-trial state bit for
bit); the reduced system at the state a rejected step returns; the chunk hand-over with the state
export on (the cost-only, exporting last K6 of a chunk on every iteration in turn, rejected ones
included) in the descriptor graph, the by-value graph and through run_async / wait; the K5
variants; the batch (one window rejecting while its neighbour accepts); the Cholesky fallback;
the sharded decision on one rank and on two P2P ranks at fold levels 1, 3 and 4.

Tolerances against the oracle are test_ba_gpu.py's: poses 1e-7, points 1e-6 m, S and b 1e-9 of
their maxima, initial cost 1e-10 relative, final cost 1e-8 of the initial cost, status and
iteration count identical.

Measured on an MI355X (largest device-versus-oracle differences over every prefix of a case;
poses / points):

    W1        4.6e-14 / 9.4e-12        W3    3.8e-11 / 1.3e-10      W4   1.2e-14 / 5.1e-14
    W2 d=2    1.4e-13 / 2.5e-11        W3b   2.4e-13 / 2.7e-12      W5   1.9e-10 / 1.7e-08
    W2 d=.05  4.7e-14 / 3.7e-10        W2 d=2 at the batch's 30 iterations: 9.0e-14 / 6.1e-08

The two largest are the reference's own spread (its 1-thread and 5-thread sums are 8.8e-9 apart
on W5's third step and 6.8e-8 on W2's 30 iterations, test_ba_lm_paths_cpu.py).  Reduced system
after a reject: S within 1.1e-12, b 2.3e-11, cost 7.4e-12 (W3) at the oracle's state; 1.1e-14,
1.2e-13, 2.7e-16 at one common state (W5).  Batch members equal their single-handle solves bit for
bit except the 4-keyframe window beside 12-keyframe ones (4.1e-16 / 1.1e-14).  The file takes
about 15 s, 10 s of it process start-up of the three two-rank runs and the RCCL communicator.
"""
import dataclasses
import time

import numpy as np
import pytest

import test_ba_lm_paths_cpu as L
from test_ba_last_iteration_gpu import _exporting, _handle, _same

pytestmark = pytest.mark.gpu

SWEEP = ["W1", "W2_d2", "W2_d005", "W3", "W3b", "W4", "W5"]


def _cfg(name, **over):
    from rsvio.ba import lm_cfg
    return lm_cfg(**{**L.CASES[name][1], **over})


def _run(ba, cfg, use_async=False):
    if use_async:
        ba.run_async(cfg)
        r = ba.wait()
    else:
        r = ba.run(cfg)
    pose, pw = ba.state()
    return (r.status, r.iterations, r.final_cost), pose.copy(), pw.copy(), r.initial_cost


def _fresh(prob, cfg):
    """The solve on a fresh handle that never turned the export on (state(): device copy)."""
    ba = _handle(prob)
    out = _run(ba, cfg)
    ba.close()
    for a in out[1:3]:
        a.setflags(write=False)
    return out


def _check_oracle(got, po, pwo, ro, tag=""):
    """test_ba_gpu.py's tolerances; returns the pose and point differences."""
    (status, iters, final), pose, pw, initial = got
    dp, dw = np.abs(pose - po).max(), np.abs(pw - pwo).max()
    print(f"{tag}: status {status} it {iters}  poses {dp:.1e}  points {dw:.1e}  "
          f"cost {abs(final - ro.final_cost) / ro.initial_cost:.1e}")
    assert (status, iters) == (ro.status, ro.iterations), tag
    assert abs(initial - ro.initial_cost) <= 1e-10 * ro.initial_cost, tag
    assert abs(final - ro.final_cost) <= 1e-8 * ro.initial_cost, tag
    assert dp < 1e-7 and dw < 1e-6, tag
    return dp, dw


class _Sweeps:
    """Per case and k = 1..K (K the oracle's iteration count): the max_iterations=k solve on a
    fresh handle and the oracle's, computed once and never modified."""

    def __init__(self, oracle):
        self.oracle = oracle
        self._dev, self._orc = {}, {}

    def dev(self, name, k):
        if (name, k) not in self._dev:
            self._dev[name, k] = _fresh(L.window(L.CASES[name][0]), _cfg(name, max_iterations=k))
        return self._dev[name, k]

    def orc(self, name, k):
        if (name, k) not in self._orc:
            cfg = self.oracle.lm_cfg(**{**L.CASES[name][1], "max_iterations": k})
            self._orc[name, k] = self.oracle.ba_solve(L.window(L.CASES[name][0]), cfg)
        return self._orc[name, k]

    def full(self, name):
        return self.dev(name, L.CASES[name][3])


@pytest.fixture(scope="module")
def sweeps(gpu, oracle):
    oracle.set_ba_threads(1)
    return _Sweeps(oracle)


@pytest.mark.parametrize("name", SWEEP)
def test_prefix_sweep(gpu, sweeps, name):
    """max_iterations = 1..K on fresh handles: every prefix equals the oracle's, the accept pattern
    derived from the device alone (step k rejected iff final_cost did not move, bit for bit) is
    the pinned one, and a prefix that ends on a step that was not applied -- rejected, or the one
    a tolerance ended the solve in -- returns the state of the prefix before it bit for bit."""
    win, _, status, K, pinned = L.CASES[name]
    prob = L.window(win)
    pat, worst = "", (0.0, 0.0)
    for k in range(1, K + 1):
        got = sweeps.dev(name, k)
        d = _check_oracle(got, *sweeps.orc(name, k), tag=f"{name} k={k}")
        worst = (max(worst[0], d[0]), max(worst[1], d[1]))
        prev = sweeps.dev(name, k - 1) if k > 1 else ((0, 0, got[3]), prob.pose7, prob.p_W, got[3])
        kept = got[0][2] == prev[0][2]
        if k <= len(pinned):
            assert got[0][0] == 3
            pat += "R" if kept else "A"
        else:       # the iteration the solve ends in: its candidate is not applied
            assert k == K and got[0][0] == status != 3 and kept
        if kept:
            assert np.array_equal(got[1], prev[1]) and np.array_equal(got[2], prev[2]), k
        else:
            assert not np.array_equal(got[2], prev[2]), k
    print(f"{name}: device pattern {pat}  worst poses {worst[0]:.1e}  points {worst[1]:.1e}")
    assert pat == pinned
    assert got[0][:2] == (status, K)


def _system_matches(oracle, prob, state_dev, state_orc, lam, delta, tag):
    at_dev = dataclasses.replace(prob, pose7=np.ascontiguousarray(state_dev[0]), p_W=np.ascontiguousarray(state_dev[1]))
    at_orc = dataclasses.replace(prob, pose7=state_orc[0], p_W=state_orc[1])
    ba = _handle(at_dev)
    S, b, cost = ba.build_system(lam, delta)
    ba.close()
    So, bo, co = oracle.ba_build_system(at_orc, lam, delta)
    print(f"{tag}: S {np.abs(S - So).max() / np.abs(So).max():.1e}  b {np.abs(b - bo).max() / np.abs(bo).max():.1e}  "
          f"cost {abs(cost - co) / abs(co):.1e}")
    assert np.abs(S - So).max() <= 1e-9 * np.abs(So).max(), tag
    assert np.abs(b - bo).max() <= 1e-9 * np.abs(bo).max(), tag
    assert abs(cost - co) <= 1e-10 * abs(co), tag


@pytest.mark.parametrize("name", ["W1", "W2_d2", "W3", "W5"])
def test_system_after_reject(gpu, oracle, sweeps, name):
    """The reduced system at the state every prefix that ends on a rejected step returns, against
    the oracle's system at the oracle's state of that prefix (L.SYSTEM_AT_ORACLE_STATE) and at
    the device's own state (every window: the same input to both, so the kernels alone are
    compared).  W5 is checked in the second form only: the oracle's own two summation orders
    leave its state after the third step 8.8e-9 apart in one weakly observed landmark and their
    systems 3.6e-10 apart in cost, more than the 1e-10 bound (test_ba_lm_paths_cpu.py)."""
    win, cfg, _, _, pinned = L.CASES[name]
    ks = [k + 1 for k, c in enumerate(pinned) if c == "R"]
    assert ks
    for k in ks:
        got, orc = sweeps.dev(name, k), sweeps.orc(name, k)
        delta = cfg.get("huber_delta", 2.0)
        _system_matches(oracle, L.window(win), got[1:3], got[1:3], 1e-4, delta, f"{name} k={k} same state")
        if name in L.SYSTEM_AT_ORACLE_STATE:
            _system_matches(oracle, L.window(win), got[1:3], orc[:2], 1e-4, delta, f"{name} k={k} oracle's state")


@pytest.mark.parametrize("delta", [0.05, 2.0])
def test_system_with_outliers_at_initial_state(gpu, oracle, delta):
    """W2's system at the initial state: a tenth of the residuals down-weighted at delta 0.05."""
    prob = L.window("W2")
    _system_matches(oracle, prob, (prob.pose7, prob.p_W), (prob.pose7, prob.p_W), 1e-4, delta, f"W2 delta {delta}")


def _hand_over(sweeps, name, ks):
    """With the export on, a max_iterations=k solve leaves the first-chunk guess at k; the full
    solve after it then runs its cost-only, exporting K6 on iteration k (and, the guess being
    short, that iteration's full K6 again).  Every solve equals the one on a fresh handle without
    the export bit for bit: in the descriptor graph (a newly set window), in the by-value graph (a
    re-solve) and through run_async / wait."""
    prob = L.window(L.CASES[name][0])
    want = sweeps.full(name)
    assert want[0][:2] == L.CASES[name][2:4]
    ba = _exporting(prob)
    for k in ks:
        short, full = _cfg(name, max_iterations=k), _cfg(name)
        for mode in ("descriptor", "by value", "async"):
            assert _same(_run(ba, short)[:3], sweeps.dev(name, k)[:3]), (k, mode, "prefix")
            if mode == "descriptor":
                ba.set_problem_from(prob)
            got = _run(ba, full, use_async=mode == "async")
            assert got[0] == want[0], (k, mode, got[0], want[0])
            assert _same(got[:3], want[:3]), (k, mode)
    ba.close()


@pytest.mark.parametrize("name", ["W1", "W2_d2", "W3", "W3b", "W5"])
def test_chunk_hand_over_on_every_iteration(gpu, sweeps, name):
    _hand_over(sweeps, name, range(1, L.CASES[name][3] + 1))


def test_new_handle_lean_k6_on_rejected_third_step(gpu, sweeps):
    """W1 on a brand-new exporting handle: the first chunk is 3 iterations and W1 rejects exactly
    its third step, so the chunk's cost-only K6 evaluates a trial that is then rejected, and the
    solve goes on from the untouched current buffer."""
    assert L.CASES["W1"][4][:3] == "AAR"
    want = sweeps.full("W1")
    ba = _exporting(L.window("W1"))
    got = _run(ba, _cfg("W1"))
    assert got[0] == want[0] and _same(got[:3], want[:3])
    ba.close()
    ba = _exporting(L.window("W1"))          # and cut off there: status 3 on the rejected step
    got = _run(ba, _cfg("W1_max3"))
    assert got[0][:2] == L.CASES["W1_max3"][2:4] and _same(got[:3], sweeps.dev("W1", 3)[:3])
    before = sweeps.dev("W1", 2)             # the state the rejected trial started from
    assert got[0][2] == before[0][2] and np.array_equal(got[1], before[1]) and np.array_equal(got[2], before[2])
    ba.close()


@pytest.mark.parametrize("variant", ["pipe4", "gj1"])
def test_camera_solve_variants_on_w1(gpu, sweeps, monkeypatch, variant):
    """The K5 A/B variants (RSVIO_K5, read at handle creation) through W1's rejected step."""
    monkeypatch.setenv("RSVIO_K5", variant)
    full = _fresh(L.window("W1"), _cfg("W1"))
    cut = _fresh(L.window("W1"), _cfg("W1_max3"))
    monkeypatch.delenv("RSVIO_K5")
    _check_oracle(full, *sweeps.orc("W1", L.CASES["W1"][3]), tag=f"W1 {variant}")
    _check_oracle(cut, *sweeps.orc("W1", 3), tag=f"W1 max 3 {variant}")


BATCHES = {
    "small": (["W1", "default5_30", "W2_d2_30", None], 1e-10),
    "past10": (["W3_30", "W5", "default4_30"], 1e-9),
}


@pytest.mark.parametrize("which", list(BATCHES))
def test_batch_with_rejecting_members(gpu, oracle, which):
    """One launch chain, one LM state per window: windows that reject steps next to windows that
    accept every step (and one the guards skip), under the batch's max_iterations=30.  Each equals
    its single-handle solve within the existing batch tests' bounds and the oracle within the
    tolerances above; run twice (the second run re-uses the chunk size)."""
    from rsvio.ba import BundleBatch, lm_cfg
    names, bound = BATCHES[which]
    cfg = lm_cfg(max_iterations=30)
    probs = [L.window(L.CASES[n][0]) if n else L.window("skipped2") for n in names]
    for n in names:
        assert n is None or {"huber_delta": 2.0, **L.CASES[n][1]} == {"huber_delta": 2.0, "max_iterations": 30}
    wins = [_handle(pr) for pr in probs]
    batch = BundleBatch(wins)
    singles = [_fresh(pr, cfg) if n else None for n, pr in zip(names, probs)]
    oracles = [oracle.ba_solve(pr, oracle.lm_cfg(max_iterations=30)) if n else None for n, pr in zip(names, probs)]
    for rep in range(2):
        for w, pr in zip(wins, probs):
            w.set_problem_from(pr)
        res = batch.run(cfg)
        for n, w, r, one, orc in zip(names, wins, res, singles, oracles):
            if n is None:
                assert r.status == -2
                continue
            pose, pw = w.state()
            assert (r.status, r.iterations) == one[0][:2] == L.CASES[n][2:4], (n, rep)
            d1 = (np.abs(pose - one[1]).max(), np.abs(pw - one[2]).max())
            print(f"{n} run {rep}: batch vs single  poses {d1[0]:.1e}  points {d1[1]:.1e}")
            _check_oracle(((r.status, r.iterations, r.final_cost), pose, pw, r.initial_cost), *orc,
                          tag=f"batch {n} run {rep}")
            assert d1[0] <= bound and d1[1] <= bound, (n, rep)
    batch.close()
    for w in wins:
        w.close()


def test_cholesky_fallback_through_a_reject(gpu, oracle, sweeps):
    """W1 with linear_solver=SOLVER_CHOLESKY: the oracle's dense full-system solve (96 landmarks)
    takes the pinned path; the device's fallback matches it and the Schur solve on the device."""
    from rsvio.ba import SOLVER_CHOLESKY
    assert L.CASES["W1_chol"][1]["linear_solver"] == SOLVER_CHOLESKY
    got = _fresh(L.window("W1"), _cfg("W1_chol"))
    assert got[0][:2] == L.CASES["W1_chol"][2:4]
    _check_oracle(got, *oracle.ba_solve(L.window("W1"), oracle.lm_cfg(**L.CASES["W1_chol"][1])), tag="W1 cholesky")
    schur = sweeps.full("W1")
    assert np.abs(got[1] - schur[1]).max() < 1e-9 and np.abs(got[2] - schur[2]).max() < 1e-8


@pytest.mark.parametrize("name", ["W1", "W3"])
def test_sharded_decision_single_rank(gpu, sweeps, name):
    """The sharded path (pre-reduced LM decision) on a one-rank communicator through rejected
    steps: bit-equal to the unsharded solve."""
    from rsvio.ba import BundleAdjuster
    prob = L.window(L.CASES[name][0])
    want = sweeps.full(name)
    b = BundleAdjuster(max_keyframes=21, max_landmarks=prob.n_lm, max_observations=prob.n_obs)
    b.attach_comm(1, 0, BundleAdjuster.rccl_unique_id())
    b.set_problem_from(prob)
    got = _run(b, _cfg(name))
    b.close()
    assert got[0] == want[0] and _same(got[:3], want[:3])


def _p2p_w3_worker(rank, world, port, out_dir, env):
    import datetime
    import os

    import torch.distributed as dist
    os.environ["RSVIO_P2P_FOLD"] = "1"   # ranks share one GPU (test_ba_gpu.py's _p2p_worker)
    os.environ.update(env or {})
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        from rsvio.ba import BundleAdjuster, lm_cfg
        shard = L.window("W3").shard(rank, world)
        ba = BundleAdjuster(max_keyframes=21, max_landmarks=shard.n_lm, max_observations=shard.n_obs)
        mine = ba.p2p_export(world)
        handles = [None] * world
        dist.all_gather_object(handles, mine)
        ba.attach_p2p(world, rank, handles)
        ba.set_problem_from(shard)
        r = ba.run(lm_cfg(**L.CASES["W3"][1]))
        pose, pw = ba.state()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), pose=pose, pw=pw,
                 res=np.array([r.status, r.iterations, r.final_cost, r.initial_cost]))
        ba.close()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _run_p2p_w3(out_dir, env, limit=120.0):
    """Two ranks on W3 (96 landmarks each); the processes are killed at the time limit."""
    import socket

    import torch.multiprocessing as mp
    out_dir.mkdir()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.start_processes(_p2p_w3_worker, args=(2, port, str(out_dir), env), nprocs=2, join=False,
                             start_method="spawn")
    deadline = time.monotonic() + limit
    while not ctx.join(timeout=1.0):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("a P2P rank did not finish within its time limit")
    return [np.load(out_dir / f"r{r}.npz") for r in range(2)]


@pytest.fixture(scope="module")
def p2p_fold1(gpu, tmp_path_factory):
    return _run_p2p_w3(tmp_path_factory.mktemp("p2p") / "fold1", {"RSVIO_P2P_FOLD": "1"})


def test_sharded_p2p_two_ranks_reject(gpu, oracle, sweeps, p2p_fold1):
    """W3 sharded over two P2P ranks: the decision's sums are exchanged, so both ranks must reject
    the same two steps; they end bit-equal, and the gathered solution matches the oracle."""
    r0, r1 = p2p_fold1
    assert np.array_equal(r0["pose"], r1["pose"]) and np.array_equal(r0["res"], r1["res"])
    po, pwo, ro = sweeps.orc("W3", L.CASES["W3"][3])
    got = ((int(r0["res"][0]), int(r0["res"][1]), float(r0["res"][2])), r0["pose"],
           np.concatenate([r0["pw"], r1["pw"]]), float(r0["res"][3]))
    assert got[0][:2] == L.CASES["W3"][2:4]
    _check_oracle(got, po, pwo, ro, tag="W3 two ranks")


@pytest.mark.parametrize("level", ["3", "4"])
def test_sharded_p2p_fold_levels_reject(gpu, tmp_path, p2p_fold1, level):
    """The 3-launch iterations (fold levels 3 and 4, as test_sharded_p2p_fold_equals_separate_exchange
    sets them) through W3's rejected steps: bit-equal to the 4-launch one on every rank."""
    sep = _run_p2p_w3(tmp_path / "sep", {"RSVIO_P2P_FOLD": level, "RSVIO_P2P_FOLD_SHARED": "1"})
    for a, b in zip(p2p_fold1, sep):
        for k in ("pose", "pw", "res"):
            assert np.array_equal(a[k], b[k]), k
