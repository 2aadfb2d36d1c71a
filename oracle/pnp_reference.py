"""A plain high-precision reference of track_motion (B8: the map join, the PnP factors with
Huber(delta), the build's LM loop) in numpy longdouble, on rotation matrices.

Test infrastructure.  It shares no code with ba_oracle.cpp (whose path goes through unit
quaternions, a Cholesky on doubles and sequential sums): the join is a searchsorted, the update
R' = R Exp(w), t' = t + R V(w) rho in closed form with no series switch, the solve a dense 6x6
Cholesky in longdouble.  What it restates on purpose is the LM loop of orc_track_motion, check by
check, because the sequence of decisions is the thing under test:

    each iteration:  cost finite?  ->  solve (H + lambda I) dx = -g  ->  parameter tolerance with
    |x|^2 = |t|^2 + 1  ->  trial pose  ->  cost tolerance |dcost| <= tol cost (before the accept
    test, whatever the sign)  ->  accept (rho > 0): lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2
    ->  else lambda *= nu, nu *= 2, stop at lambda > 1e32.

Every iteration leaves a log entry with the quantities each decision compared, so a test can
require that no outcome of an input hangs on rounding (tests/test_motion_reference_cpu.py).

Also here: the restatement of pnp.hip's host hash table (map_bucket, the table-size rule, the
insertion) that the join cases of oracle/pnp_cases.py are built with.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

LD = np.longdouble

LM_COST_TOL, LM_PARAM_TOL, LM_MAX_ITERS, LM_TRUST_REGION = 1, 2, 3, 4
LM_NUMFAIL, LM_SKIPPED, LM_LINSOLVE = -1, -2, -3


@dataclass
class RefIteration:
    """What one LM iteration compared.  Fields a stopped iteration never computed are None."""
    param_ratio: float            # |dx| / (tol (|x| + tol)); <= 1 stops with LM_PARAM_TOL
    cost_ratio: float | None      # |dcost| / (tol cost); <= 1 stops with LM_COST_TOL
    rho: float | None             # the gain ratio dcost / predicted
    angle: float                  # |w| of the step (rad)
    accepted: bool | None


@dataclass
class RefMotionResult:
    status: int
    iterations: int
    n_observations: int
    initial_cost: float
    final_cost: float
    T_W_B: np.ndarray             # 4x4 longdouble; identity when the optimisation failed
    log: list = field(default_factory=list)


def _hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], LD)


def _exp_so3(w):
    """Exp(w) and the left Jacobian V(w), closed forms."""
    th2 = w @ w
    K = _hat(w)
    I = np.eye(3, dtype=LD)
    if th2 == 0:
        return I, I
    th = np.sqrt(th2)
    A = np.sin(th) / th
    sh = np.sin(th / 2)
    B = 2 * sh * sh / th2
    Cc = (th - np.sin(th)) / (th2 * th)
    KK = K @ K
    return I + A * K + B * KK, I + B * K + Cc * KK


def _system(R, t, obs, TCB, delta):
    """H, g and cost = sum rho / 2 over the factors, left then right, at T_B_W = (R, t)."""
    H = np.zeros((6, 6), LD)
    g = np.zeros(6, LD)
    cost = LD(0)
    d = LD(delta)
    for c in (0, 1):
        pW, uv = obs[c]
        if len(pW) == 0:
            continue
        Rcw = TCB[c][:3, :3] @ R
        tcw = TCB[c][:3, :3] @ t + TCB[c][:3, 3]
        pC = pW @ Rcw.T + tcw
        iz = 1 / pC[:, 2]
        x = pC[:, 0] * iz
        y = pC[:, 1] * iz
        r = np.stack([x - uv[:, 0], y - uv[:, 1]], 1)
        J = np.zeros((len(pW), 2, 6), LD)
        J[:, 0, :3] = iz[:, None] * (Rcw[0] - x[:, None] * Rcw[2])
        J[:, 1, :3] = iz[:, None] * (Rcw[1] - y[:, None] * Rcw[2])
        for i in range(2):
            J[:, i, 3:] = -np.cross(J[:, i, :3], pW)      # dw_i = -(dt_i x p_W)
        s = (r * r).sum(1)
        out = ~(s <= d * d)                                # NaN goes the outer way, as in C
        sq = np.sqrt(np.where(out, s, LD(1)))
        rho = np.where(out, 2 * d * sq - d * d, s)
        w = np.where(out, d / sq, LD(1))
        cost += rho.sum() / 2
        H += np.einsum("n,nia,nib->ab", w, J, J)
        g += np.einsum("n,nia,ni->a", w, J, r)
    return H, g, cost


def _chol_solve(A, b):
    """x of A x = b by Cholesky in longdouble; None when a pivot is not positive and finite."""
    n = len(b)
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not (d > 0 and np.isfinite(d)):
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    z = np.zeros(n, LD)
    for i in range(n):
        z[i] = (b[i] - L[i, :i] @ z[:i]) / L[i, i]
    x = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        x[i] = (z[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def join(ids, map_ids):
    """(mask of the features with a map point, their map rows); map_ids ascending."""
    ids = np.asarray(ids, np.uint64).reshape(-1)
    map_ids = np.asarray(map_ids, np.uint64).reshape(-1)
    if len(map_ids) == 0 or len(ids) == 0:
        return np.zeros(len(ids), bool), np.zeros(0, np.int64)
    k = np.minimum(np.searchsorted(map_ids, ids), len(map_ids) - 1)
    ok = map_ids[k] == ids
    return ok, k[ok]


def track_motion_ref(ids_l, uv_l, ids_r, uv_r, map_ids, map_pw, T_W_B_last_kf, T_C_B2, cfg=None) -> RefMotionResult:
    """cfg: a mapping with any of max_iterations (10), cost_tolerance (1e-6), parameter_tolerance
    (1e-9), huber_delta (2.0), lambda_init (1e-4)."""
    cfg = dict(cfg or {})
    max_it = int(cfg.get("max_iterations", 10))
    ctol = LD(cfg.get("cost_tolerance", 1e-6))
    ptol = LD(cfg.get("parameter_tolerance", 1e-9))
    delta = cfg.get("huber_delta", 2.0)
    lam = LD(cfg.get("lambda_init", 1e-4))
    map_pw = np.asarray(map_pw, np.float32).reshape(-1, 3)
    obs = []
    for ids, uv in ((ids_l, uv_l), (ids_r, uv_r)):
        uv = np.asarray(uv, np.float32).reshape(-1, 2)
        ok, rows = join(ids, map_ids)
        obs.append((map_pw[rows].astype(LD), uv[ok].astype(LD)))
    n_obs = len(obs[0][0]) + len(obs[1][0])
    I4 = np.eye(4, dtype=LD)
    if n_obs == 0:
        return RefMotionResult(LM_SKIPPED, 0, 0, 0.0, 0.0, I4)
    TCB = [np.asarray(T_C_B2, np.float64).reshape(2, 4, 4)[c].astype(LD) for c in (0, 1)]
    Tl = np.asarray(T_W_B_last_kf, np.float64).reshape(4, 4).astype(LD)
    R = Tl[:3, :3].T.copy()                                # T_B_W = inv(T_W_B_last_kf)
    t = -R @ Tl[:3, 3]
    log = []
    with np.errstate(all="ignore"):
        H, g, cost = _system(R, t, obs, TCB, delta)
        cost0 = cost
        nu = LD(2)
        status, it = LM_MAX_ITERS, 0
        for it in range(1, max_it + 1):
            if not np.isfinite(cost):
                status = LM_NUMFAIL
                break
            dx = _chol_solve(H + lam * np.eye(6, dtype=LD), -g)
            if dx is None:
                status = LM_LINSOLVE
                break
            dx2 = dx @ dx
            e = RefIteration(float(np.sqrt(dx2) / (ptol * (np.sqrt(t @ t + 1) + ptol))), None, None,
                             float(np.sqrt(dx[3:] @ dx[3:])), None)
            log.append(e)
            if np.sqrt(dx2) <= ptol * (np.sqrt(t @ t + 1) + ptol):
                status = LM_PARAM_TOL
                break
            E, V = _exp_so3(dx[3:])
            Rt = R @ E
            tt = t + R @ (V @ dx[:3])
            Ht, gt, new_cost = _system(Rt, tt, obs, TCB, delta)
            pred = (lam * dx2 - g @ dx) / 2
            dcost = cost - new_cost
            rho = dcost / pred
            e.cost_ratio = float(abs(dcost) / (ctol * cost))
            e.rho = float(rho)
            if np.isfinite(new_cost) and abs(dcost) <= ctol * cost:
                status = LM_COST_TOL
                break
            if np.isfinite(new_cost) and rho > 0:
                e.accepted = True
                R, t, H, g, cost = Rt, tt, Ht, gt, new_cost
                f = 2 * rho - 1
                lam = lam * max(LD(1) / 3, 1 - f * f * f)
                nu = LD(2)
            else:
                e.accepted = False
                lam = lam * nu
                nu = nu * 2
                if lam > LD(1e32):
                    status = LM_TRUST_REGION
                    break
    T = I4.copy()
    if status > 0:
        T[:3, :3] = R.T
        T[:3, 3] = -R.T @ t
    return RefMotionResult(status, it, n_obs, float(cost0), float(cost), T, log)


# ---- the host hash table of pnp.hip (rsvio_pnp_set_map), restated ------------------------------

TOP_ID = (1 << 64) - 1      # the free-entry marker: a map point with this id is carried beside the table
BUCKET = 4                  # entries per bucket
_GOLD = 0x9E3779B97F4A7C15


def map_bucket(id_, mask):
    """Fibonacci hashing: ((id * 0x9E3779B97F4A7C15 mod 2^64) >> 40) & mask."""
    return (((int(id_) * _GOLD) & TOP_ID) >> 40) & mask


def map_bucket_array(ids, mask):
    with np.errstate(over="ignore"):
        return ((np.asarray(ids, np.uint64) * np.uint64(_GOLD)) >> np.uint64(40)) & np.uint64(mask)


def table_buckets(n):
    """The smallest power of two >= 16 with at least n buckets (4 n entries: load <= 1/4)."""
    nb = 16
    while nb < n:
        nb *= 2
    return nb


def build_table(map_ids):
    """The insertion of set_map (ids ascending, linear probing over buckets).  Returns
    dict(buckets, max_probe, has_top, n_map, depth={id: the probe depth it was stored at})."""
    ids = sorted(int(i) for i in map_ids)
    nb = table_buckets(len(ids))
    fill = [0] * nb
    depth, has_top, max_probe = {}, 0, 0
    for i in ids:
        if i == TOP_ID:
            has_top = 1
            continue
        b, p = map_bucket(i, nb - 1), 0
        while fill[b] == BUCKET:
            b, p = (b + 1) & (nb - 1), p + 1
        fill[b] += 1
        depth[i] = p
        max_probe = max(max_probe, p)
    return dict(buckets=nb, max_probe=max_probe, has_top=has_top, n_map=len(ids), depth=depth, fill=fill)


def lookup_depth(id_, table, stored):
    """How a lookup of id_ ends in `table` (build_table's) holding the ids `stored`: ('hit', p),
    ('free', p) -- a miss ended by a bucket with a free entry at depth p -- or ('exhausted', p) --
    a miss that walked the whole run of max_probe + 1 full buckets."""
    nb = table["buckets"]
    if int(id_) == TOP_ID:
        return ("hit", 0) if table["has_top"] else ("free", 0)
    b = map_bucket(id_, nb - 1)
    where = {}
    for i in stored:
        i = int(i)
        if i != TOP_ID:
            where[i] = (map_bucket(i, nb - 1) + table["depth"][i]) & (nb - 1)
    for p in range(table["max_probe"] + 1):
        if where.get(int(id_)) == b:
            return ("hit", p)
        if table["fill"][b] < BUCKET:
            return ("free", p)
        b = (b + 1) & (nb - 1)
    return ("exhausted", table["max_probe"])
