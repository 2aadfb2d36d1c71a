"""The camera system's symbolic envelope (rs-vio_amd/csrc/ba_envelope.hpp) on the CPU.

Past 10 free keyframes rsvio_ba_set_problem hands the solver env[k], the last block row of column
block k that may be non-zero: the Schur chunks outside it write zeros and the 6x6-block LDL^T skips
the tiles outside it, so an envelope that is too small drops terms silently.
tools/ba_envelope_dump.cpp compiles the header with g++ and prints the envelopes of the patterns
it reads; the reference here is numpy: the block pattern "some landmark sees the free keyframes a
and b" and its symbolic block elimination in column order.  The named patterns of
rsvio.synthetic (the windows of tests/test_ba_envelope_gpu.py) are pinned here too.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_MAX_FREE = 20
NAMES = ["two_ended", "full_span", "random_gaps", "staircase", "two_fixed_mono"]


@pytest.fixture(scope="module")
def dump_bin(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ absent")
    out = str(tmp_path_factory.mktemp("env") / "ba_envelope_dump")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rs-vio_amd", "csrc"),
                    os.path.join(ROOT, "tools", "ba_envelope_dump.cpp"), "-o", out], check=True)
    return out


def _envelopes(dump_bin, cases):
    """cases: [(see (n_lm, n_kf, 2) bool, fixed (n_kf,) bool)] -> [(env_on, env (20,))] of the header."""
    lines = [str(len(cases))]
    for see, fixed in cases:
        n_lm, n_kf, _ = see.shape
        w = 1 << (2 * np.arange(n_kf, dtype=object)[:, None] + np.arange(2, dtype=object)[None, :])
        lines.append(f"{n_kf} {n_lm}")
        lines.append(" ".join(str(int(f)) for f in fixed))
        lines.append(" ".join(format(int((see[l] * w).sum()), "x") for l in range(n_lm)))
    r = subprocess.run([dump_bin], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [[int(x) for x in ln.split()] for ln in r.stdout.strip().splitlines()]
    assert len(rows) == len(cases) and all(len(x) == 1 + K_MAX_FREE for x in rows)
    return [(x[0], np.array(x[1:])) for x in rows]


def _free_vis(see, fixed):
    """(n_lm, n_free) bool: landmark l is seen (by either camera) from free keyframe a."""
    return see.any(2)[:, ~np.asarray(fixed, bool)]


def _pattern(fv):
    """Block pattern of S: P[a, b] = some landmark sees the free keyframes a and b (+ the diagonal)."""
    f = fv.astype(np.int64)
    return ((f.T @ f) > 0) | np.eye(fv.shape[1], dtype=bool)


def _filled_last_row(P):
    """Symbolic block elimination in column order; the last non-zero block row of every column of
    the filled pattern (= of L)."""
    F = P.copy()
    n = F.shape[0]
    for k in range(n):
        rows = np.nonzero(F[k + 1:, k])[0] + k + 1
        F[np.ix_(rows, rows)] = True
    return np.array([np.nonzero(F[:, k])[0].max() for k in range(n)])


def _raw_candidates(fv):
    """cand[a] = the last free keyframe of the landmarks whose first free keyframe is a (-1: none)."""
    cand = np.full(fv.shape[1], -1)
    for row in fv:
        ks = np.nonzero(row)[0]
        if len(ks):
            cand[ks[0]] = max(cand[ks[0]], ks[-1])
    return cand


def _check(see, fixed, env_on, env, tag):
    fv = _free_vis(see, fixed)
    n_free = fv.shape[1]
    assert np.array_equal(env[n_free:], np.arange(n_free, K_MAX_FREE)), tag
    if n_free <= 10:
        assert env_on == 0 and np.all(env[:n_free] == n_free - 1), tag
        return
    assert env_on == 1, tag
    k = np.arange(n_free)
    assert np.all(env[:n_free] >= k) and np.all(env[:n_free] <= n_free - 1), tag
    last = _filled_last_row(_pattern(fv))
    assert np.all(last <= env[:n_free]), (tag, last, env[:n_free])
    restated = np.maximum(k, np.maximum.accumulate(_raw_candidates(fv)))
    assert np.array_equal(env[:n_free], restated), (tag, env[:n_free], restated)


def _named(name, n_kf):
    from rsvio import synthetic as S
    vis, cam, fixed = S.pattern_visibility(name, n_kf)
    see = vis[:, :, None] & (np.ones(vis.shape + (2,), bool) if cam is None else cam)
    fx = np.zeros(n_kf, bool)
    fx[list(fixed)] = True
    return see, fx


def _see_of(prob):
    see = np.zeros((prob.n_lm, prob.n_kf, 2), bool)
    see[prob.obs_lm, prob.obs_kf, prob.obs_cam] = True
    return see


def test_named_patterns_every_size(dump_bin):
    """The five named patterns at every n_free from 11 to 20 (and below the threshold, where the
    envelope is off and dense)."""
    tags, cases = [], []
    for name in NAMES:
        n_fixed = 2 if name == "two_fixed_mono" else 1
        for n_free in list(range(5, 11)) + list(range(11, 21)):
            tags.append((name, n_free))
            cases.append(_named(name, n_free + n_fixed))
    for tag, (see, fixed), (on, env) in zip(tags, cases, _envelopes(dump_bin, cases)):
        assert (~fixed).sum() == tag[1]
        _check(see, fixed, on, env, tag)


def test_random_visibility(dump_bin):
    """A few hundred random windows: random fixed sets (interior ones included), sparse and dense
    landmarks, left-only and right-only keyframes, landmarks seen from fixed keyframes only and
    landmarks with no observation."""
    rng = np.random.default_rng(4815)
    cases = []
    for i in range(400):
        n_kf = int(rng.integers(12, 22)) if i % 4 else int(rng.integers(2, 13))
        n_fixed = int(rng.integers(max(1, n_kf - K_MAX_FREE), min(4, n_kf) + 1)) if n_kf > 2 else 1
        fixed = np.zeros(n_kf, bool)
        fixed[rng.choice(n_kf, n_fixed, replace=False)] = True
        n_lm = int(rng.integers(1, 40))
        see = np.zeros((n_lm, n_kf, 2), bool)
        width = int(rng.integers(2, n_kf + 1))           # how far apart a landmark's keyframes may lie
        for l in range(n_lm):
            kind = rng.integers(0, 10)
            if kind == 0:
                continue                                  # no observation at all
            if kind == 1:
                ks = np.nonzero(fixed)[0]                 # fixed keyframes only
            else:
                lo = int(rng.integers(0, n_kf - width + 1))
                ks = lo + rng.choice(width, int(rng.integers(1, min(width, 6) + 1)), replace=False)
            for k in ks:
                see[l, k] = [(True, True), (True, False), (False, True)][int(rng.integers(0, 3))]
        cases.append((see, fixed))
    seen_on = 0
    for i, ((see, fixed), (on, env)) in enumerate(zip(cases, _envelopes(dump_bin, cases))):
        _check(see, fixed, on, env, i)
        seen_on += on
    assert seen_on >= 200


def test_staircase_envelope_is_strictly_inside_the_dense_one(dump_bin):
    for n_kf in (12, 14, 17, 21):
        see, fixed = _named("staircase", n_kf)
        (on, env), = _envelopes(dump_bin, [(see, fixed)])
        n_free = n_kf - 1
        assert on == 1 and 2 * (env[:n_free] < n_free - 1).sum() >= n_free, env
        assert len(set(env[:n_free] - np.arange(n_free))) >= 3  # edges at several offsets


def test_two_ended_needs_the_prefix_maximum(dump_bin):
    """two_ended's raw per-start maxima are not monotone: env[k] = max(k, cand[k]) without the
    running maximum would lie below the filled pattern."""
    for n_kf in (11, 12, 14, 15, 17, 21):
        see, fixed = _named("two_ended", n_kf)
        fv = _free_vis(see, fixed)
        n_free = fv.shape[1]
        cand = _raw_candidates(fv)
        assert cand[0] == n_free - 1 and np.any(np.diff(cand) < 0)
        naive = np.maximum(np.arange(n_free), cand)
        assert np.any(naive < _filled_last_row(_pattern(fv)))
        if n_free > 10:
            (on, env), = _envelopes(dump_bin, [(see, fixed)])
            assert np.all(env[:n_free] == n_free - 1)


def test_right_only_keyframe_counts(dump_bin):
    """A landmark whose last keyframe has only the right camera still couples that keyframe (the
    m2 | m2 >> 1 fold): two_fixed_mono's envelope equals the one of the same window with both
    cameras everywhere."""
    see, fixed = _named("two_fixed_mono", 14)
    both = np.repeat(see.any(2)[:, :, None], 2, 2)
    (on_a, env_a), (on_b, env_b) = _envelopes(dump_bin, [(see, fixed), (both, fixed)])
    assert on_a == on_b == 1 and np.array_equal(env_a, env_b)
    left_only = see & np.array([True, False])
    (_, env_l), = _envelopes(dump_bin, [(left_only, fixed)])
    assert np.any(env_l < env_a)  # (dropping the right-only keyframes does shrink it)


@pytest.mark.parametrize("n_kf", [14, 21])
def test_staircase_shards_have_smaller_envelopes(dump_bin, oracle, n_kf):
    """A landmark-sharded solve factors the all-reduced system of every rank's landmarks: the
    envelope of shard 0 of 2 alone lies strictly below the whole window's in some column, and the
    oracle's S has a non-zero block there -- the solver must not factor with its own shard's."""
    from rsvio import synthetic as S
    prob = S.ba_pattern_problem("staircase", n_kf)
    fixed = prob.kf_fixed.astype(bool)
    (_, env), (_, env0), (_, env1) = _envelopes(
        dump_bin, [(_see_of(prob), fixed), (_see_of(prob.shard(0, 2)), fixed), (_see_of(prob.shard(1, 2)), fixed)])
    n_free = n_kf - 1
    assert np.all(env0 <= env) and np.all(env1 <= env)
    So, _, _ = oracle.ba_build_system(prob, 1e-4)
    blk = np.abs(So.reshape(n_free, 6, n_free, 6)).max((1, 3)) > 0
    last = np.array([np.nonzero(blk[:, k])[0].max() for k in range(n_free)])
    assert np.all(last <= env[:n_free])
    assert np.any(last > env0[:n_free]), (last, env0)


def test_generator_follows_the_visibility():
    from rsvio import synthetic as S
    prob = S.ba_pattern_problem("two_fixed_mono", 12)
    see, fixed = _named("two_fixed_mono", 12)
    assert prob.n_obs == see.sum() and np.array_equal(_see_of(prob), see)
    assert np.array_equal(prob.kf_fixed.astype(bool), fixed) and fixed[[0, 5]].all() and fixed.sum() == 2
    assert np.array_equal(prob.pose7[fixed], prob.true_pose7[fixed])
    assert np.all(np.abs(prob.pose7[~fixed] - prob.true_pose7[~fixed]).max(1) > 0)
    assert np.array_equal(prob.obs_uv, prob.obs_uv.astype(np.float32).astype(np.float64))
    key = (prob.obs_lm.astype(np.int64) << 6) | (prob.obs_kf << 1) | prob.obs_cam
    assert np.all(np.diff(key) > 0)                      # landmark-major, no duplicate
    assert not see[-1].any() and see[-3:-1].any(2)[:, ~fixed].sum() == 0 and see[-3:-1].any()
