"""A plain numpy f64 restatement of the robust motion tracking contract (include/rsvio_gpu.h,
rsvio_track_motion_robust): R1 the join by searchsorted, the pairs and their triangulation, R2 the
sampler, the triangle pose and the inlier counts, R3 the selection.  The refit is the oracle's
track_motion on the inlier-filtered lists, started from the winner's pose (given as inv(T_B_W) in
place of T_W_B_last_kf); the keyframe figures are recomputed against the real last keyframe.

Every squared error that was compared with the threshold is returned (RefRobust.sq_errors), so a
test can check that none lies within rounding of it (margin_ok): the device composes T_C_B T_B_W
before it multiplies and sums in another order, which moves an error by a few ulp.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

M64 = (1 << 64) - 1
OK, TOO_FEW_PAIRS, NO_CONSENSUS = 1, 2, -1
LM_SKIPPED = -2


def splitmix64_at(seed: int, i: int) -> int:
    z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_indices(seed: int, n_hyp: int, n_pairs: int) -> np.ndarray:
    """The seeded sampler's n_hyp x 3 pair indices (row 0 unused: -1; n_pairs 0: all -1)."""
    s = np.full((n_hyp, 3), -1, np.int64)
    if n_pairs > 0:
        for h in range(1, n_hyp):
            for k in range(3):
                s[h, k] = splitmix64_at(seed, 3 * h + k) % n_pairs
    return s


@dataclass
class Joined:
    w: np.ndarray      # n x 3 map points (f32 widened)
    uv: np.ndarray     # n x 2
    cam: np.ndarray    # n
    pos: np.ndarray    # n, position in the camera's list
    n_l: int
    n_r: int


def join(ids_l, uv_l, ids_r, uv_r, map_ids, map_pw) -> Joined:
    map_ids = np.asarray(map_ids, np.uint64)
    map_pw = np.asarray(map_pw, np.float32).reshape(-1, 3)
    w, uv, cam, pos = [], [], [], []
    for c, (ids, u) in enumerate(((ids_l, uv_l), (ids_r, uv_r))):
        ids = np.asarray(ids, np.uint64).reshape(-1)
        u = np.asarray(u, np.float32).reshape(-1, 2)
        if len(map_ids) and len(ids):
            at = np.searchsorted(map_ids, ids)
            at_c = np.minimum(at, len(map_ids) - 1)
            hit = (at < len(map_ids)) & (map_ids[at_c] == ids)
        else:
            at_c = np.zeros(len(ids), np.int64)
            hit = np.zeros(len(ids), bool)
        idx = np.nonzero(hit)[0]
        w.append(map_pw[at_c[idx]].astype(np.float64).reshape(-1, 3))
        uv.append(u[idx].astype(np.float64))
        cam.append(np.full(len(idx), c, np.int64))
        pos.append(idx.astype(np.int64))
    return Joined(np.concatenate(w), np.concatenate(uv), np.concatenate(cam), np.concatenate(pos),
                  len(np.asarray(ids_l).reshape(-1)), len(np.asarray(ids_r).reshape(-1)))


def find_pairs(J: Joined, ids_l, ids_r):
    """(k_left, k_right): indices into the joined observations of each pair, by ascending left
    position; the mate is the FIRST joined right feature with the same id."""
    ids_l = np.asarray(ids_l, np.uint64).reshape(-1)
    ids_r = np.asarray(ids_r, np.uint64).reshape(-1)
    first_right = {}
    for k in np.nonzero(J.cam == 1)[0]:
        first_right.setdefault(int(ids_r[J.pos[k]]), int(k))
    kl, kr = [], []
    for k in np.nonzero(J.cam == 0)[0]:
        m = first_right.get(int(ids_l[J.pos[k]]))
        if m is not None:
            kl.append(int(k))
            kr.append(m)
    return np.asarray(kl, np.int64), np.asarray(kr, np.int64)


def triangulate_pair(T_C_B2, uv_left, uv_right, min_depth):
    """q in the body frame by the least-squares intersection of the two rays, and its validity."""
    T = np.asarray(T_C_B2, np.float64).reshape(2, 4, 4)
    A = np.zeros((3, 3))
    r = np.zeros(3)
    for c, uv in enumerate((uv_left, uv_right)):
        R, t = T[c, :3, :3], T[c, :3, 3]
        centre = -R.T @ t
        d = R.T @ np.array([uv[0], uv[1], 1.0])
        d = d / np.linalg.norm(d)
        M = np.eye(3) - np.outer(d, d)
        A += M
        r += M @ centre
    det = np.linalg.det(A)
    if not (det > 1e-12 * 8.0) or not np.isfinite(det):
        return np.zeros(3), False
    q = np.linalg.solve(A, r)
    if not np.all(np.isfinite(q)):
        return q, False
    ok = all((T[c, :3, :3] @ q + T[c, :3, 3])[2] >= min_depth for c in range(2))
    return q, bool(ok)


def triangle_frame(p):
    a, b = p[1] - p[0], p[2] - p[0]
    n = np.cross(a, b)
    aa, bb, nn = a @ a, b @ b, n @ n
    if not (nn > 1e-12 * (aa * bb)):
        return None
    e1 = a / math.sqrt(aa)
    e3 = n / math.sqrt(nn)
    e2 = np.cross(e3, e1)
    return np.stack([e1, e2, e3], 1)


def triangle_pose(w3, q3):
    """(R, t) of T_B_W with q = R w + t on the two triangles, or None when either is degenerate."""
    w3, q3 = np.asarray(w3, np.float64), np.asarray(q3, np.float64)
    Fw, Fq = triangle_frame(w3), triangle_frame(q3)
    if Fw is None or Fq is None:
        return None
    R = Fq @ Fw.T
    t = q3.mean(0) - R @ w3.mean(0)
    if not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
        return None
    return R, t


def classify(R, t, J: Joined, T_C_B2, sq, min_depth):
    """(inlier flags, squared errors, depths) of every joined observation at T_B_W = [R | t]."""
    T = np.asarray(T_C_B2, np.float64).reshape(2, 4, 4)
    if len(J.w) == 0:
        return np.zeros(0, bool), np.zeros(0), np.zeros(0)
    pb = J.w @ R.T + t
    pc = np.einsum("nij,nj->ni", T[J.cam, :3, :3], pb) + T[J.cam, :3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        e = pc[:, :2] / pc[:, 2:3] - J.uv
        e2 = (e * e).sum(1)
        inl = (pc[:, 2] >= min_depth) & (e2 <= sq)
    return inl, e2, pc[:, 2]


def rigid_inverse(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    Ti = np.eye(4)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return Ti


def rot_of_quat(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (w * y + x * z)],
                     [2 * (w * z + x * y), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (w * x + y * z), w * w - x * x - y * y + z * z]])


def euler_norm(R):
    """|(roll, pitch, yaw)| of Rotation3::euler_angles (estimator.rs:207-216)."""
    if abs(R[2, 0]) < 1.0:
        pitch = -math.asin(R[2, 0])
        c = math.cos(pitch)
        roll = math.atan2(R[2, 1] / c, R[2, 2] / c)
        yaw = math.atan2(R[1, 0] / c, R[0, 0] / c)
    elif R[2, 0] <= -1.0:
        roll, pitch, yaw = math.atan2(R[0, 1], R[0, 2]), math.pi / 2, 0.0
    else:
        roll, pitch, yaw = -math.atan2(-R[0, 1], -R[0, 2]), -math.pi / 2, 0.0
    return math.sqrt(roll * roll + pitch * pitch + yaw * yaw)


@dataclass
class RefRobust:
    ransac_status: int
    n_pairs: int
    n_valid_pairs: int
    n_valid_hyp: int
    best_hyp: int
    best_count: int
    n_inliers: int
    hyp_count: np.ndarray
    mask_l: np.ndarray
    mask_r: np.ndarray
    status: int
    iterations: int
    n_observations: int
    is_keyframe: int
    T_W_B: np.ndarray
    initial_cost: float
    final_cost: float
    translation_norm: float
    rotation_norm: float
    winner_mask: np.ndarray                 # inlier flags of the joined observations at the winner's pose
    best_is_unique: bool
    tied: list = field(default_factory=list)      # the hypotheses sharing the best count
    tied_same_set: bool = True              # ... all with the winner's inlier SET (the refit cannot tell them apart)
    sq_errors: list = field(default_factory=list)  # every array of squared errors compared with the threshold


def robust_track_motion(oracle, ids_l, uv_l, ids_r, uv_r, map_ids, map_pw, T_W_B_last_kf, T_C_B2, n_hyp=256,
                        min_inliers=10, seed=0, inlier_sq_error=1e-4, min_depth=0.1, samples=None, cfg=None,
                        thr_t=0.05, thr_r=0.05) -> RefRobust:
    ids_l = np.asarray(ids_l, np.uint64).reshape(-1)
    ids_r = np.asarray(ids_r, np.uint64).reshape(-1)
    uv_l = np.asarray(uv_l, np.float32).reshape(-1, 2)
    uv_r = np.asarray(uv_r, np.float32).reshape(-1, 2)
    T_last = np.asarray(T_W_B_last_kf, np.float64).reshape(4, 4)
    J = join(ids_l, uv_l, ids_r, uv_r, map_ids, map_pw)
    kl, kr = find_pairs(J, ids_l, ids_r)
    n_pairs = len(kl)
    pq = np.zeros((n_pairs, 3))
    pok = np.zeros(n_pairs, bool)
    for i in range(n_pairs):
        pq[i], pok[i] = triangulate_pair(T_C_B2, J.uv[kl[i]], J.uv[kr[i]], min_depth)
    pw = J.w[kl] if n_pairs else np.zeros((0, 3))
    if samples is None:
        samples = sample_indices(seed, n_hyp, n_pairs)
    samples = np.asarray(samples, np.int64).reshape(n_hyp, 3)
    # R2
    prior = rigid_inverse(T_last)
    poses = [(prior[:3, :3], prior[:3, 3])]
    counts = np.full(n_hyp, -1, np.int64)
    sq_all = []
    inl0, e2, _ = classify(*poses[0], J, T_C_B2, inlier_sq_error, min_depth)
    counts[0] = int(inl0.sum())
    sq_all.append(e2)
    masks = {0: inl0}
    for h in range(1, n_hyp):
        i = samples[h]
        poses.append(None)
        if n_pairs < 3 or np.any(i < 0) or np.any(i >= n_pairs) or len(set(i.tolist())) < 3 or not np.all(pok[i]):
            continue
        P = triangle_pose(pw[i], pq[i])
        if P is None:
            continue
        poses[h] = P
        inl, e2, _ = classify(*P, J, T_C_B2, inlier_sq_error, min_depth)
        counts[h] = int(inl.sum())
        sq_all.append(e2)
        masks[h] = inl
    # R3: the largest count, the lowest h on a tie
    best = int(np.argmax(counts))
    best_count = int(counts[best])
    tied = [int(h) for h in np.nonzero(counts == best_count)[0]]
    consensus = best_count >= max(min_inliers, 1)
    mask_l = np.zeros(J.n_l, np.uint8)
    mask_r = np.zeros(J.n_r, np.uint8)
    left, right = J.cam == 0, J.cam == 1
    out = RefRobust(ransac_status=NO_CONSENSUS, n_pairs=n_pairs, n_valid_pairs=int(pok.sum()),
                    n_valid_hyp=int((counts >= 0).sum()), best_hyp=best, best_count=best_count, n_inliers=0,
                    hyp_count=counts.astype(np.int32), mask_l=mask_l, mask_r=mask_r, status=LM_SKIPPED, iterations=0,
                    n_observations=0, is_keyframe=1, T_W_B=np.eye(4), initial_cost=0.0, final_cost=0.0,
                    translation_norm=0.0, rotation_norm=0.0, winner_mask=masks[best], best_is_unique=len(tied) == 1,
                    tied=tied, tied_same_set=all(np.array_equal(masks[h], masks[best]) for h in tied),
                    sq_errors=sq_all)
    if not consensus:
        mask_l[J.pos[left]] = 2
        mask_r[J.pos[right]] = 2
        return out
    out.ransac_status = TOO_FEW_PAIRS if n_pairs < 3 else OK
    win = masks[best]
    R, t = poses[best]
    if best == 0:
        T_start = T_last
    else:
        T_BW = np.eye(4)
        T_BW[:3, :3], T_BW[:3, 3] = R, t
        T_start = rigid_inverse(T_BW)
    keep_l = np.zeros(J.n_l, bool)
    keep_r = np.zeros(J.n_r, bool)
    keep_l[J.pos[left & win]] = True
    keep_r[J.pos[right & win]] = True
    kw = {} if cfg is None else {"cfg": cfg}
    o = oracle.track_motion(ids_l[keep_l], uv_l[keep_l], ids_r[keep_r], uv_r[keep_r], map_ids, map_pw, T_start,
                            T_C_B2, thr_t=thr_t, thr_r=thr_r, **kw)
    out.status, out.iterations, out.n_observations = o.status, o.iterations, o.n_observations
    out.initial_cost, out.final_cost = o.initial_cost, o.final_cost
    if o.status > 0:
        T_W_B = np.array(o.T_W_B[:]).reshape(4, 4)
        out.T_W_B = T_W_B
        T_rel = T_W_B @ rigid_inverse(T_last)
        out.translation_norm = float(np.linalg.norm(T_rel[:3, 3]))
        out.rotation_norm = euler_norm(rot_of_quat(oracle.quat_from_matrix(T_rel[:3, :3])))
        out.is_keyframe = int(out.translation_norm > thr_t or out.rotation_norm > thr_r)
        F = rigid_inverse(T_W_B)
        Rf, tf = F[:3, :3], F[:3, 3]
    else:
        Rf, tf = R, t
    fin, e2, _ = classify(Rf, tf, J, T_C_B2, inlier_sq_error, min_depth)
    out.sq_errors.append(e2)
    mask_l[J.pos[left]] = np.where(fin[left], 1, 2)
    mask_r[J.pos[right]] = np.where(fin[right], 1, 2)
    out.n_inliers = int(fin.sum())
    return out


def run_case(oracle, m, uv_l=None, uv_r=None, **kw) -> RefRobust:
    """robust_track_motion on a MotionFrame (optionally with replaced coordinates)."""
    return robust_track_motion(oracle, m.ids_l, m.uv_l if uv_l is None else uv_l, m.ids_r,
                               m.uv_r if uv_r is None else uv_r, m.map_ids, m.map_pw, m.T_W_B_last_kf, m.T_C_B2, **kw)


# The corrupted frame of tests/test_robust_motion_cpu.py, shared with the GPU test: the seed of the
# sampler and the threshold were chosen on the CPU so that the winner's consensus set is exactly
# the labelled inliers (corruptions are >= 0.05 away, i.e. >= 2.5e-3 squared; clean residuals at
# 0.3 px are ~1e-6), and the LM is run to convergence so that two starts reach the same pose
CORRUPT_SQ = 1e-3
CORRUPT_SEED = 0
CORRUPT_HYP = 256
CORRUPT_LM = dict(max_iterations=30, cost_tolerance=1e-12, parameter_tolerance=1e-12)


def corrupted_frame(frac: float = 0.3, rng_seed: int = 1234):
    """motion_frame(n_map=400, n_feat=120, noise_px=0.3, map_noise=0.001) with a chosen `frac` of
    its joined observations displaced by an offset of norm in [0.05, 0.5] -> (frame, uv_l, uv_r,
    labels_l, labels_r); labels: 0 no map point, 1 clean, 2 displaced."""
    from rsvio import synthetic as S
    m = S.motion_frame(n_map=400, n_feat=120, noise_px=0.3, map_noise=0.001, seed=3)
    J = join(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.map_ids, m.map_pw)
    rng = np.random.default_rng(rng_seed)
    bad = np.sort(rng.choice(len(J.w), int(round(frac * len(J.w))), replace=False))
    uv = [m.uv_l.copy(), m.uv_r.copy()]
    lab = [np.zeros(J.n_l, np.uint8), np.zeros(J.n_r, np.uint8)]
    for c in range(2):
        lab[c][J.pos[J.cam == c]] = 1
    for k in bad:
        ang, nrm = rng.uniform(0.0, 2.0 * math.pi), rng.uniform(0.05, 0.5)
        uv[J.cam[k]][J.pos[k]] += (nrm * np.array([math.cos(ang), math.sin(ang)])).astype(np.float32)
        lab[J.cam[k]][J.pos[k]] = 2
    return m, uv[0], uv[1], lab[0], lab[1]


def margin_ok(ref: RefRobust, sq: float, rel: float = 1e-9) -> bool:
    """No compared squared error -- of any hypothesis or of the final classification -- within `rel`
    (relative) of the threshold: every inlier decision, hence every count, survives the device's
    different rounding."""
    for e2 in ref.sq_errors:
        e2 = e2[np.isfinite(e2)]
        if np.any(np.abs(e2 - sq) <= rel * sq):
            return False
    return True


def winner_ok(ref: RefRobust) -> bool:
    """The winner is unique, or tied only by construction: every hypothesis sharing the best count
    has the winner's inlier set (identical sample rows, permutations of one triple, several
    hypotheses that each capture every clean observation, or nothing at all), so the tie rule
    (lowest h) picks among equals."""
    return ref.best_is_unique or ref.tied_same_set
