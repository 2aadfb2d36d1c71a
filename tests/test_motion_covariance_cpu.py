"""The motion covariance's definition on the CPU (tests/motion_covariance_reference.py, no device):
the tangent and the sign of the Jacobian the Hessian is built from, the conditioning of the frames
the GPU parity test uses, and the reference's handling of masks."""
import numpy as np
import pytest

import motion_covariance_reference as R
from oracle.pnp_reference import LD, _exp_so3, _system

EPS = float(np.finfo(np.float64).eps)


def _frame(**kw):
    from rsvio import synthetic as S
    m = S.motion_frame(**kw)
    return m, (m.ids_l, m.uv_l, m.ids_r, m.uv_r), (m.map_ids, m.map_pw)


def _exp_se3(d):
    """The LM's Exp([dt; dw]) as a 4x4 (se3_plus_r: rotation Exp(dw), translation V(dw) dt)."""
    E, V = _exp_so3(d[3:])
    T = np.eye(4, dtype=LD)
    T[:3, :3] = E
    T[:3, 3] = V @ d[:3]
    return T


def _inv(T):
    Ti = np.eye(4, dtype=LD)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return Ti


def test_tangent_and_sign_by_central_differences():
    """Central differences (h = 1e-5: truncation O(h^2) = 1e-10 of the second derivative, four orders
    below the 1e-6 tolerance) of the stacked residuals under T_B_W Exp(h e_k) reproduce _system's J --
    through H = J^T J and g = J^T r at an inactive Huber delta, g fixing the sign -- and the same
    residuals under Exp(-h e_k) T_W_B give the same columns: the covariance is T_W_B's under a left
    perturbation."""
    m, lists, map_ = _frame()
    obs = R.factors(lists, map_)
    TCB = R.tcb_of(m.T_C_B2)
    T_W_B = np.asarray(m.T_W_B_true, np.float64).astype(LD)
    T_B_W = _inv(T_W_B)
    h = LD(1e-5)

    def res(T):
        return R.residuals(T[:3, :3], T[:3, 3], obs, TCB).reshape(-1)

    J_right = np.zeros((len(res(T_B_W)), 6), LD)
    J_left = np.zeros_like(J_right)
    for k in range(6):
        e = np.zeros(6, LD)
        e[k] = h
        J_right[:, k] = (res(T_B_W @ _exp_se3(e)) - res(T_B_W @ _exp_se3(-e))) / (2 * h)
        J_left[:, k] = (res(_inv(_exp_se3(-e) @ T_W_B)) - res(_inv(_exp_se3(e) @ T_W_B))) / (2 * h)
    scale = np.abs(J_right).max(0)
    assert float((np.abs(J_left - J_right) / scale).max()) <= 1e-6
    H, g, _ = _system(T_B_W[:3, :3], T_B_W[:3, 3], obs, TCB, 1e9)
    r0 = res(T_B_W)
    d = np.sqrt(np.diag(H))
    assert float((np.abs(J_right.T @ J_right - H) / np.outer(d, d)).max()) <= 1e-6
    assert float((np.abs(J_right.T @ r0 - g) / np.abs(g).max()).max()) <= 1e-6
    assert float(np.abs(g).max()) > 0


@pytest.mark.parametrize("name", list(R.PARITY_FRAMES))
def test_parity_frames_are_well_conditioned(name):
    """kappa(H_ref) <= 1e3 at both Huber deltas, so the reference's own error bound 5 eps kappa 6 is
    below the GPU test's cap with margin."""
    m, lists, map_ = _frame(**R.PARITY_FRAMES[name])
    for delta in (2.0, 0.002):
        H, S, _, n, _ = R.reference(lists, map_, m.T_W_B_true, m.T_C_B2, delta)
        kappa = float(np.linalg.cond(H))
        print(f"{name} delta {delta}: n {n} kappa {kappa:.1f}")
        assert kappa <= R.KAPPA_MAX
        assert 5 * EPS * kappa * 6 <= R.PARITY_CAP
        assert np.abs(S @ H - np.eye(6)).max() <= 5 * EPS * kappa * 6


def test_three_factor_frame_is_outside_the_parity_bound():
    """The 3-factor frame (checked on the GPU by its residual, not by parity) must not slip into the
    parity list: its conditioning is past the list's bound, masked down to 3 factors or not."""
    m, lists, map_ = _frame(n_feat=3, unmapped=0)
    assert len(m.ids_l) == 3 and len(m.ids_r) == 3
    masks = (np.ones(3, np.uint8), np.zeros(3, np.uint8))
    for mk, n_want in ((masks, 3), (None, 6)):
        H, S, _, n, _ = R.reference(lists, map_, m.T_W_B_true, m.T_C_B2, 2.0, mk)
        kappa = float(np.linalg.cond(H))
        print(f"{n} factors: kappa {kappa:.3g}")
        assert n == n_want and S is not None
        assert kappa > R.KAPPA_MAX
    assert dict(n_feat=3, unmapped=0) not in R.PARITY_FRAMES.values()


def test_reference_masks():
    m, lists, map_ = _frame(n_feat=40, outlier_frac=0.2)
    args = (lists, map_, m.T_W_B_true, m.T_C_B2, 0.002)
    H0, S0, c0, n0, d0 = R.reference(*args)
    ones = (np.ones(len(m.ids_l), np.uint8), np.ones(len(m.ids_r), np.uint8))
    H1, S1, c1, n1, d1 = R.reference(*args, ones)
    assert np.array_equal(H0, H1) and np.array_equal(S0, S1) and (c0, n0, d0) == (c1, n1, d1)
    assert n0 == len(m.ids_l) + len(m.ids_r) - 80 and 0 < d0 <= n0     # (40 unmapped per camera)
    zeros = (np.zeros(len(m.ids_l), np.uint8), np.zeros(len(m.ids_r), np.uint8))
    H2, S2, c2, n2, d2 = R.reference(*args, zeros)
    assert n2 == 0 and d2 == 0 and S2 is None and c2 == 0.0 and not H2.any()
    # 2 (the robust call's outlier mark) is not 1; a 1 on a feature without a map point is ignored
    twos = (np.full(len(m.ids_l), 2, np.uint8), None)
    assert R.reference(*args, twos)[3] == int(R.factors(lists, map_)[1][0].shape[0])
