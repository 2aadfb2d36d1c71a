"""The two reference routes of the covariance tests (tests/test_covariance_{cpu,gpu}.py), both
evaluated at a given state of a synthetic BAProblem:

* schur_pose_cov: numpy's inverse of the oracle's reduced camera system S at lambda = 0;
* dense_cov: the camera and landmark blocks of numpy's inverse of the whole Gauss-Newton Hessian
  H = sum w J^T J (6 n_free + 3 n_lm square), assembled here from oracle.factor_linearize per
  observation with the Huber weight restated -- no Schur formula anywhere.

scaled_err is the tests' metric: max_ij |A - R|_ij / sqrt(R_ii R_jj)."""
import dataclasses

import numpy as np


def at_state(prob, pose7, p_W):
    """The problem with its initial state replaced by (pose7, p_W)."""
    return dataclasses.replace(prob, pose7=np.ascontiguousarray(pose7, np.float64).copy(),
                               p_W=np.ascontiguousarray(p_W, np.float64).reshape(-1, 3).copy())


def scaled_err(a, ref):
    d = np.sqrt(np.diag(ref))
    return float(np.max(np.abs(a - ref) / np.outer(d, d)))


def schur_pose_cov(oracle, prob, huber_delta=2.0):
    S, _, _ = oracle.ba_build_system(prob, 0.0, huber_delta)
    return np.linalg.inv(S)


def dense_cov(oracle, prob, huber_delta=2.0):
    """(pose covariance n x n, landmark covariances n_lm x 3 x 3, observed n_lm bool) from inv(H);
    a landmark without observations has no rows in H and zeros here."""
    fixed = np.asarray(prob.kf_fixed) != 0
    free_idx = np.full(prob.n_kf, -1)
    free_idx[~fixed] = np.arange(int((~fixed).sum()))
    nc = 6 * int((~fixed).sum())
    observed = np.zeros(prob.n_lm, bool)
    observed[np.asarray(prob.obs_lm)] = True
    lm_col = np.full(prob.n_lm, -1)
    lm_col[observed] = nc + 3 * np.arange(int(observed.sum()))
    H = np.zeros((nc + 3 * int(observed.sum()),) * 2)
    for o in range(prob.n_obs):
        l, k, c = int(prob.obs_lm[o]), int(prob.obs_kf[o]), int(prob.obs_cam[o])
        r, J = oracle.factor_linearize(prob.p_W[l], prob.pose7[k], prob.T_C_B2[c], prob.obs_uv[o])
        s = float(r @ r)
        w = 1.0 if s <= huber_delta * huber_delta else huber_delta / np.sqrt(s)
        cols = list(range(lm_col[l], lm_col[l] + 3))
        Jv = [J[:, 0:3]]
        if free_idx[k] >= 0:
            cols += list(range(6 * free_idx[k], 6 * free_idx[k] + 6))
            Jv.append(J[:, 3:9])
        Jv = np.concatenate(Jv, axis=1)
        H[np.ix_(cols, cols)] += w * (Jv.T @ Jv)
    Hi = np.linalg.inv(H)
    lm = np.zeros((prob.n_lm, 3, 3))
    for l in np.nonzero(observed)[0]:
        lm[l] = Hi[lm_col[l]:lm_col[l] + 3, lm_col[l]:lm_col[l] + 3]
    return Hi[:nc, :nc], lm, observed
