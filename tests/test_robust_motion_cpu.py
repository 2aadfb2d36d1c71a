"""The numpy reference of robust motion tracking (tests/robust_motion_reference.py) on its own: the
sampler, the triangle pose, the pair triangulation, and the whole pipeline on a frame with 30 % of
its observations displaced.  The GPU test compares the device with this reference; this file pins
the reference."""
import functools
import math

import numpy as np

import robust_motion_reference as R


def _splitmix_scalar(seed, i):
    """A second implementation: numpy uint64 scalars with wrapping arithmetic."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * np.uint64(i + 1)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return int(z ^ (z >> np.uint64(31)))


def test_sampler_known_answers():
    # splitmix64's published first outputs for the state 0 (the stream i = 0, 1, 2 of seed 0)
    assert [R.splitmix64_at(0, i) for i in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    for seed in (0, 1, 0xDEADBEEF, 2 ** 64 - 1):
        for i in (0, 1, 2, 3, 17, 3071, 3 * 1023 + 2):
            assert R.splitmix64_at(seed, i) == _splitmix_scalar(seed, i)
    s = R.sample_indices(5, 8, 37)
    assert s.shape == (8, 3) and np.all(s[0] == -1) and np.all((s[1:] >= 0) & (s[1:] < 37))
    assert s[3, 1] == _splitmix_scalar(5, 3 * 3 + 1) % 37
    assert np.all(R.sample_indices(5, 4, 0) == -1)


def test_triangle_pose_recovers_a_rigid_transform():
    rng = np.random.default_rng(7)
    for _ in range(20):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        a = rng.uniform(-3.0, 3.0)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        Rt = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
        t = rng.uniform(-2, 2, 3)
        w = rng.uniform(-4, 4, (3, 3))
        q = w @ Rt.T + t
        Rh, th = R.triangle_pose(w, q)
        assert np.abs(Rh - Rt).max() <= 1e-12 and np.abs(th - t).max() <= 1e-12
        assert np.abs(Rh @ Rh.T - np.eye(3)).max() <= 1e-14
    # collinear points: no pose
    w = np.array([[0.0, 0, 0], [1, 1, 1], [2, 2, 2]])
    assert R.triangle_pose(w, w + 1.0) is None
    assert R.triangle_pose(np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), w) is None


def test_pair_triangulation():
    from rsvio import synthetic as S
    T_C_B2 = np.stack([np.linalg.inv(S.T_B_CL), np.linalg.inv(S.T_B_CR)])
    rng = np.random.default_rng(3)
    for _ in range(10):
        q = np.linalg.inv(T_C_B2[0])[:3, :3] @ np.array([rng.uniform(-2, 2), rng.uniform(-1, 1), rng.uniform(1, 8)]) + \
            np.linalg.inv(T_C_B2[0])[:3, 3]
        uv = []
        for c in range(2):
            pc = T_C_B2[c, :3, :3] @ q + T_C_B2[c, :3, 3]
            uv.append(pc[:2] / pc[2])
        qh, ok = R.triangulate_pair(T_C_B2, uv[0], uv[1], 0.1)
        assert ok and np.abs(qh - q).max() <= 1e-9
        _, ok = R.triangulate_pair(T_C_B2, uv[0], uv[1], 100.0)     # nearer than min_depth
        assert not ok
    # parallel rays: the same ray in the body frame from both cameras
    d_b = np.array([0.1, -0.05, 1.0])
    uv = []
    for c in range(2):
        d = T_C_B2[c, :3, :3] @ d_b
        uv.append(d[:2] / d[2])
    _, ok = R.triangulate_pair(T_C_B2, uv[0], uv[1], 0.1)
    assert not ok


@functools.lru_cache(maxsize=None)
def _corrupted(oracle):
    m, uv_l, uv_r, lab_l, lab_r = R.corrupted_frame()
    cfg = oracle.lm_cfg(**R.CORRUPT_LM)
    ref = R.run_case(oracle, m, uv_l, uv_r, n_hyp=R.CORRUPT_HYP, seed=R.CORRUPT_SEED, inlier_sq_error=R.CORRUPT_SQ,
                     cfg=cfg)
    fit = oracle.track_motion(m.ids_l[lab_l == 1], uv_l[lab_l == 1], m.ids_r[lab_r == 1], uv_r[lab_r == 1], m.map_ids,
                              m.map_pw, m.T_W_B_last_kf, m.T_C_B2, cfg=cfg)
    plain = oracle.track_motion(m.ids_l, uv_l, m.ids_r, uv_r, m.map_ids, m.map_pw, m.T_W_B_last_kf, m.T_C_B2, cfg=cfg)
    return m, lab_l, lab_r, ref, np.array(fit.T_W_B[:]).reshape(4, 4), np.array(plain.T_W_B[:]).reshape(4, 4)


def test_reference_separates_thirty_percent_outliers(oracle):
    """240 joined observations, 72 of them displaced by 0.05 .. 0.5 (23 .. 230 px at EuRoC's fx).
    Recorded here on the CPU: the plain track_motion (every observation, Huber 2.0 in normalised
    units) ends 6.2e-2 (max |T_W_B - truth|) away from the true pose; the robust reference, whose
    winner (h = 1, 168 inliers of 168 clean) is refit on exactly the clean observations, ends
    5.5e-4 away -- the noise floor of the clean fit, which it equals to 1e-10."""
    m, lab_l, lab_r, ref, T_fit, T_plain = _corrupted(oracle)
    n_clean = int((lab_l == 1).sum() + (lab_r == 1).sum())
    n_bad = int((lab_l == 2).sum() + (lab_r == 2).sum())
    assert n_clean + n_bad == 240 and n_bad == 72
    assert ref.ransac_status == R.OK and ref.status > 0
    assert np.array_equal(ref.mask_l, lab_l) and np.array_equal(ref.mask_r, lab_r)   # no mislabel
    assert ref.best_count == n_clean == ref.n_inliers == ref.n_observations
    assert np.abs(ref.T_W_B - T_fit).max() <= 1e-9
    err_plain = np.abs(T_plain - m.T_W_B_true).max()
    err_robust = np.abs(ref.T_W_B - m.T_W_B_true).max()
    print(f"plain {err_plain:.3e} robust {err_robust:.3e} fit diff {np.abs(ref.T_W_B - T_fit).max():.3e}")
    assert err_robust < 1e-3 < 3e-2 < err_plain


def test_margin_guard(oracle):
    """The guard every GPU case applies to its reference: no compared squared error within 1e-9
    (relative) of the threshold, and a winner that is unique (here) or tied only with hypotheses of
    the same inlier set (winner_ok)."""
    _, _, _, ref, _, _ = _corrupted(oracle)
    assert R.margin_ok(ref, R.CORRUPT_SQ) and ref.best_is_unique and R.winner_ok(ref)
    # the guard does fire: a threshold placed on one of the compared errors
    e = ref.sq_errors[0]
    on = float(e[np.isfinite(e)][0])
    assert not R.margin_ok(ref, on)
    assert not R.margin_ok(ref, on * (1 + 5e-10))
    import dataclasses
    assert not R.winner_ok(dataclasses.replace(ref, best_is_unique=False, tied_same_set=False))
    assert R.winner_ok(dataclasses.replace(ref, best_is_unique=False, tied_same_set=True))


def test_no_consensus_and_too_few_pairs(oracle):
    from rsvio import synthetic as S
    m = S.motion_frame(n_map=64, n_feat=24, seed=5)
    # every observation displaced: nothing reaches min_inliers
    rng = np.random.default_rng(0)
    uv_l, uv_r = (uv + (rng.choice([-1.0, 1.0], uv.shape) * rng.uniform(0.5, 1.5, uv.shape)).astype(np.float32)
                  for uv in (m.uv_l, m.uv_r))
    ref = R.run_case(oracle, m, uv_l, uv_r, n_hyp=64, min_inliers=10)
    assert ref.ransac_status == R.NO_CONSENSUS and ref.status == R.LM_SKIPPED and ref.is_keyframe == 1
    assert np.array_equal(ref.T_W_B, np.eye(4)) and ref.n_inliers == 0
    assert set(np.unique(ref.mask_l)) <= {0, 2}
    # the right list without a map point: no pair, only the prior is a hypothesis
    off = np.uint64(10 ** 9)
    ref = R.robust_track_motion(oracle, m.ids_l, m.uv_l, m.ids_r + off, m.uv_r, m.map_ids, m.map_pw,
                                m.T_W_B_last_kf, m.T_C_B2, n_hyp=8, inlier_sq_error=1e-2)
    assert ref.n_pairs == 0 and ref.ransac_status == R.TOO_FEW_PAIRS and ref.best_hyp == 0
    assert ref.n_valid_hyp == 1 and np.all(ref.hyp_count[1:] == -1) and ref.status > 0
