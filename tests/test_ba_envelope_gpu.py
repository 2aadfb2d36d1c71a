"""GPU parity of the BA on windows whose camera system is not a narrow band.

Past 10 free keyframes the Schur chunks and the 6x6-block LDL^T skip what lies outside the
symbolic envelope of the camera system (csrc/ba_envelope.hpp; its CPU test is
tests/test_ba_envelope_cpu.py).  synthetic.ba_problem's landmarks over consecutive keyframes give
the narrowest band only; the named patterns of rsvio.synthetic give a factor that fills in
completely (two_ended), a dense system (full_span), landmarks with gaps (random_gaps), envelope
edges at many offsets to the 16-row tiles (staircase) and an interior fixed keyframe with
one-camera keyframes, landmarks seen only from fixed keyframes and one without observations
(two_fixed_mono) -- single windows, a batch and a two-rank sharded solve.

Tolerances: those of tests/test_ba_gpu.py (S, b within 1e-9 of their maxima, cost within 1e-10
relative, the camera step within 1e-9 relative of a dense solve, poses within 1e-7, landmarks
within 1e-6 m, identical LM status and iteration count).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ["two_ended", "full_span", "random_gaps", "staircase", "two_fixed_mono"]
# n_kf 12, 14, 17, 21: 11, 13, 16, 20 free keyframes (one fewer for two_fixed_mono): the padded
# templates 13, 16 and 20; two_ended at 11 (10 free: the envelope is off) and 15 (14 free: padded to 16)
CASES = [(name, n_kf) for name in NAMES for n_kf in (12, 14, 17, 21)] + [("two_ended", 11), ("two_ended", 15)]
IDS = [f"{name}-{n_kf}" for name, n_kf in CASES]


@functools.lru_cache(maxsize=None)
def _problem(name, n_kf):
    from rsvio import synthetic as S
    return S.ba_pattern_problem(name, n_kf)


@functools.lru_cache(maxsize=None)
def _oracle_solve(name, n_kf):
    from oracle import oracle as O
    return O.ba_solve(_problem(name, n_kf))


def _adjuster(prob):
    from rsvio.ba import BundleAdjuster
    ba = BundleAdjuster(max_keyframes=21, max_landmarks=max(prob.n_lm, 1), max_observations=max(prob.n_obs, 1))
    ba.set_problem_from(prob)
    return ba


def _blocks(S):
    n = S.shape[0] // 6
    return np.abs(S.reshape(n, 6, n, 6)).max((1, 3))


def _assert_oracle_optimised(ro):
    """The comparison is not vacuous: the oracle converged over several iterations."""
    assert ro.status > 0 and ro.iterations >= 3 and ro.final_cost < 0.1 * ro.initial_cost


@pytest.mark.parametrize("lam", [1e-4, 1.0])
@pytest.mark.parametrize("name,n_kf", CASES, ids=IDS)
def test_reduced_system_matches_oracle(gpu, oracle, name, n_kf, lam):
    prob = _problem(name, n_kf)
    ba = _adjuster(prob)
    S, b, cost = ba.build_system(lam)
    ba.close()
    So, bo, co = oracle.ba_build_system(prob, lam)
    n_free = int((prob.kf_fixed == 0).sum())
    assert S.shape == So.shape == (6 * n_free, 6 * n_free)
    assert np.abs(S - So).max() <= 1e-9 * np.abs(So).max()
    assert np.abs(b - bo).max() <= 1e-9 * np.abs(bo).max()
    assert abs(cost - co) <= 1e-10 * abs(co)
    assert np.allclose(S, S.T, rtol=0, atol=1e-12 * np.abs(S).max())
    # a chunk skipped wrongly shows even where its block is small against max|S|
    missing = (_blocks(So) > 0) & ~(_blocks(S) > 0)
    assert not missing.any(), np.argwhere(missing)


@pytest.mark.parametrize("name,n_kf", CASES, ids=IDS)
def test_camera_step_matches_dense_solve(gpu, name, n_kf):
    lam = 1e-4
    ba = _adjuster(_problem(name, n_kf))
    S, b, _ = ba.build_system(lam)
    ref = np.linalg.solve(S, b)
    first = None
    for _ in range(3):
        dc = ba.camera_step(lam)
        assert np.abs(dc - ref).max() <= 1e-9 * np.abs(ref).max()
        if first is None:
            first = dc
        assert np.array_equal(dc, first)
    ba.close()


@pytest.mark.parametrize("name,n_kf", CASES, ids=IDS)
def test_solve_matches_oracle(gpu, oracle, name, n_kf):
    prob = _problem(name, n_kf)
    po, pwo, ro = _oracle_solve(name, n_kf)
    _assert_oracle_optimised(ro)
    ba = _adjuster(prob)
    res = ba.run()
    pose, pw = ba.state()
    ba.close()
    assert res.status == ro.status and res.iterations == ro.iterations
    assert np.abs(pose - po).max() < 1e-7
    assert np.abs(pw - pwo).max() < 1e-6


def test_batched_non_banded_windows(gpu, oracle):
    """Batched mode (the 6x6-block solver's padded template of 20, each window with its own
    envelope) on non-banded windows next to a 3-free-keyframe one: every window equals its own
    single-handle solve (status, iterations, state within 1e-9) and the oracle's solve."""
    from rsvio import synthetic as S
    from rsvio.ba import BundleBatch
    probs = [_problem("two_ended", 14), _problem("staircase", 17), _problem("full_span", 21),
             S.ba_problem(n_kf=4, n_lm=90, kf_per_lm=3, seed=900, init_seed=950)]
    wins = [_adjuster(pr) for pr in probs]
    batch = BundleBatch(wins)
    res = batch.run()
    for i, (w, pr, r) in enumerate(zip(wins, probs, res)):
        pose, pw = w.state()
        one = _adjuster(pr)
        r1 = one.run()
        p1, w1 = one.state()
        one.close()
        assert (r.status, r.iterations) == (r1.status, r1.iterations), i
        assert np.abs(pose - p1).max() <= 1e-9 and np.abs(pw - w1).max() <= 1e-9, i
        po, pwo, ro = oracle.ba_solve(pr)
        assert ro.status > 0
        assert r.status == ro.status and r.iterations == ro.iterations, i
        assert np.abs(pose - po).max() < 1e-7 and np.abs(pw - pwo).max() < 1e-6, i
    batch.close()
    for w in wins:
        w.close()


def _p2p_pattern_worker(rank, world, port, out_dir, name, n_kf):
    """One rank of a landmark-sharded solve of a named pattern (contiguous landmark ranges)."""
    import os

    import torch.distributed as dist
    os.environ["RSVIO_P2P_FOLD"] = "1"  # (ranks share one GPU: see test_ba_gpu._p2p_worker)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from rsvio.ba import BundleAdjuster
        shard = _problem(name, n_kf).shard(rank, world)
        ba = BundleAdjuster(max_keyframes=21, max_landmarks=shard.n_lm, max_observations=shard.n_obs)
        mine = ba.p2p_export(world)
        handles = [None] * world
        dist.all_gather_object(handles, mine)
        ba.attach_p2p(world, rank, handles)
        ba.set_problem_from(shard)
        r = ba.run()
        pose, pw = ba.state()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), pose=pose, pw=pw,
                 res=np.array([r.status, r.iterations, r.final_cost, r.initial_cost]))
        ba.close()
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n_kf", [14, 21])
def test_sharded_p2p_past_ten_free_keyframes(gpu, oracle, tmp_path, n_kf):
    """Two ranks past 10 free keyframes on staircase, whose contiguous shards have different
    envelopes, each smaller than the whole window's (test_ba_envelope_cpu): every rank factors the
    all-reduced system of both, so the solver must take an envelope that covers both.  Both ranks
    bit-equal; the gathered solution matches the oracle's single-problem solve."""
    import socket

    import torch.multiprocessing as mp
    po, pwo, ro = _oracle_solve("staircase", n_kf)
    _assert_oracle_optimised(ro)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.start_processes(_p2p_pattern_worker, args=(2, port, str(tmp_path), "staircase", n_kf), nprocs=2, join=True,
                       start_method="spawn")
    r0, r1 = np.load(tmp_path / "r0.npz"), np.load(tmp_path / "r1.npz")
    assert np.array_equal(r0["pose"], r1["pose"]) and np.array_equal(r0["res"], r1["res"])
    assert int(r0["res"][0]) == ro.status and int(r0["res"][1]) == ro.iterations
    assert abs(r0["res"][2] - ro.final_cost) <= 1e-8 * ro.initial_cost
    assert np.abs(r0["pose"] - po).max() < 1e-7
    assert np.abs(np.concatenate([r0["pw"], r1["pw"]]) - pwo).max() < 1e-6
