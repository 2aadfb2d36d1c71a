"""The motion covariance (rsvio_motion_covariance*) in numpy longdouble.  Not a test.

The definition of include/rsvio_gpu.h, restated on oracle/pnp_reference.py's pieces: the factors are
the features with a map point (`join`) whose mask byte is 1, H = sum w J^T J with no damping at
T_B_W = inverse(T_W_B) (`_system`: J the PnP factor's 2x6 [dt | dw], w the Huber IRLS weight), the
covariance numpy's inverse of H.
"""
import numpy as np

from oracle.pnp_reference import LD, _system, join

MCOV_OK, MCOV_TOO_FEW, MCOV_SINGULAR = 1, -1, -2

# The GPU parity cases: rsvio.synthetic.motion_frame arguments and the Huber deltas each runs at
# (0.002: the weights are active).  test_motion_covariance_cpu.py bounds every frame's conditioning.
PARITY_FRAMES = {
    "n8": dict(n_feat=8),                                    # 16 factors, less than one wave
    "n64": dict(n_feat=64),                                  # a full wave per camera + the unmapped tail
    "n65": dict(n_feat=65),                                  # one past the wave boundary
    "default": dict(),                                       # 600 factors + 80 unmapped: a second stride round
    "outliers": dict(outlier_frac=0.3),                      # many weights below 1
    "capacity": dict(n_map=2048, n_feat=2048, unmapped=0),   # 4,096 features: the capacity edge
}
PARITY_DELTAS = {"n8": (2.0,), "n64": (2.0,), "n65": (2.0,), "default": (2.0, 0.002), "outliers": (2.0, 0.002),
                 "capacity": (2.0,)}
PARITY_CAP = 1e-8       # on the scaled error of Sigma
KAPPA_MAX = 1e3         # of H_ref on every parity frame
KNEE_MARGIN = 1e-9      # no factor this close (relative) to the Huber knee where counts are compared


def pose_of(T_W_B):
    """(R, t) of T_B_W = inverse(T_W_B), longdouble."""
    T = np.asarray(T_W_B, np.float64).reshape(4, 4).astype(LD)
    R = T[:3, :3].T.copy()
    return R, -R @ T[:3, 3]


def tcb_of(T_C_B2):
    return [np.asarray(T_C_B2, np.float64).reshape(2, 4, 4)[c].astype(LD) for c in (0, 1)]


def factors(frame_lists, map_, masks=None):
    """[(p_W, uv) left, (p_W, uv) right] of the factors, longdouble, in list order."""
    ids_l, uv_l, ids_r, uv_r = frame_lists
    map_ids, map_pw = map_
    map_pw = np.asarray(map_pw, np.float32).reshape(-1, 3)
    masks = masks or (None, None)
    obs = []
    for ids, uv, m in ((ids_l, uv_l, masks[0]), (ids_r, uv_r, masks[1])):
        ids = np.asarray(ids, np.uint64).reshape(-1)
        uv = np.asarray(uv, np.float32).reshape(-1, 2)
        ok, rows = join(ids, map_ids)
        use = np.ones(len(ids), bool) if m is None else np.asarray(m, np.uint8).reshape(-1) == 1
        obs.append((map_pw[rows][use[ok]].astype(LD), uv[ok & use].astype(LD)))
    return obs


def residuals(R, t, obs, TCB):
    """The stacked residuals (n, 2) of the factors at T_B_W = (R, t), left then right."""
    out = []
    for c in (0, 1):
        pW, uv = obs[c]
        Rcw = TCB[c][:3, :3] @ R
        tcw = TCB[c][:3, :3] @ t + TCB[c][:3, 3]
        pC = pW.reshape(-1, 3) @ Rcw.T + tcw
        out.append(pC[:, :2] / pC[:, 2:3] - uv.reshape(-1, 2))
    return np.concatenate(out, 0)


def knee_margin(frame_lists, map_, T_W_B, T_C_B2, delta, masks=None):
    """The smallest |s - delta^2| / delta^2 over the factors (s the squared residual): how far the
    nearest factor is from the Huber knee."""
    obs = factors(frame_lists, map_, masks)
    R, t = pose_of(T_W_B)
    r = residuals(R, t, obs, tcb_of(T_C_B2))
    if len(r) == 0:
        return np.inf
    d2 = LD(delta) * LD(delta)
    return float(np.abs((r * r).sum(1) - d2).min() / d2)


def reference(frame_lists, map_, T_W_B, T_C_B2, delta, masks=None):
    """(H, Sigma, cost, n, n_down): the 6x6 Hessian (summed in longdouble, returned as float64) and
    numpy.linalg.inv of it (None below 3 factors), the cost sum rho / 2, the number of factors and
    of those beyond the Huber knee (w < 1)."""
    obs = factors(frame_lists, map_, masks)
    n = len(obs[0][0]) + len(obs[1][0])
    R, t = pose_of(T_W_B)
    TCB = tcb_of(T_C_B2)
    with np.errstate(all="ignore"):
        H, _, cost = _system(R, t, obs, TCB, delta)
        r = residuals(R, t, obs, TCB)
        n_down = int((~((r * r).sum(1) <= LD(delta) * LD(delta))).sum())
    if n < 3:
        return np.asarray(H, np.float64), None, float(cost), n, n_down
    H = np.asarray(H, np.float64)
    with np.errstate(all="ignore"):
        Sigma = np.linalg.inv(H) if np.isfinite(H).all() else np.full((6, 6), np.nan)
    return H, Sigma, float(cost), n, n_down


def scaled_error(S, S_ref):
    """max |S - S_ref|_ij / sqrt(S_ref,ii S_ref,jj) (tests/test_covariance_gpu.py's metric)."""
    d = np.sqrt(np.diag(S_ref))
    return float(np.max(np.abs(S - S_ref) / np.outer(d, d)))
