"""numpy reference of the tracker's stereo gate (include/rsvio_gpu.h, rsvio_tracker_set_stereo_gate).

The contract restated, every sum written out left to right in f64:
  essential(T)            E = [t / |t|]x R of a 4 x 4 T_Cl_Cr (x_l = R x_r + t)
  bearings(uv, conv)      unit bearings of stored f32 coordinates, PLANE (0) or RAY (1), and their validity
  gate_lists(...)         the join of two ascending-id lists, e = |d_l . (E d_r)| and the decision
and the two twin rules as set logic on the lists of an ungated tracker fed the same images:
  drop_both_lists         the twin's lists minus the rejected ids (the twin then removes them)
  DropRight               left = the never-gated twin's left; right = its right minus the accumulated R(t)
gated_oracle_run() applies gate_lists to the CPU oracle tracker (DROP_BOTH through its remove_ids,
DROP_RIGHT through DropRight) and is what pins the test sequences' splits."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

PLANE, RAY = 0, 1
DROP_RIGHT, DROP_BOTH = 1, 2


def essential(T) -> np.ndarray:
    T = np.asarray(T, np.float64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    n = np.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
    h = t / n
    S = np.array([[0.0, -h[2], h[1]], [h[2], 0.0, -h[0]], [-h[1], h[0], 0.0]])
    E = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            E[i, j] = S[i, 0] * R[0, j] + S[i, 1] * R[1, j] + S[i, 2] * R[2, j]
    return E


def bearings(uv, convention: int):
    """(n x 3 f64 bearings, valid) of n x 2 stored f32 coordinates; rows of invalid entries are NaN."""
    uv = np.asarray(uv, np.float32).reshape(-1, 2).astype(np.float64)
    x, y = uv[:, 0], uv[:, 1]
    valid = ~(np.isnan(x) | np.isnan(y))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if convention == RAY:
            s = (1.0 - x * x) - y * y
            valid &= ~(s < 0.0)
            d = np.stack([x, y, np.sqrt(np.where(s < 0.0, np.nan, s))], 1)
        else:
            n = np.sqrt((x * x + y * y) + 1.0)
            d = np.stack([x / n, y / n, 1.0 / n], 1)
    d[~valid] = np.nan
    return d, valid


def pair_error(E, dl, dr):
    """e = |d_l . (E d_r)| row by row, both products left-to-right sums."""
    v = [E[k, 0] * dr[:, 0] + E[k, 1] * dr[:, 1] + E[k, 2] * dr[:, 2] for k in range(3)]
    return np.abs(dl[:, 0] * v[0] + dl[:, 1] * v[1] + dl[:, 2] * v[2])


@dataclass
class GateResult:
    keep_l: np.ndarray      # bool per left entry
    keep_r: np.ndarray      # bool per right entry
    err_r: np.ndarray       # e per right entry; NaN: unpaired or invalid
    n_pairs: int
    n_rejected: int
    n_invalid: int
    rejected_ids: np.ndarray   # ascending
    rejected_err: np.ndarray   # their e (NaN: invalid)
    margin: float              # min |e - max_error| / max_error over the valid pairs (inf without one)


def gate_lists(T, max_error, mode, conv_l, conv_r, ids_l, uv_l, ids_r, uv_r) -> GateResult:
    E = essential(T)
    ids_l, ids_r = np.asarray(ids_l, np.uint64), np.asarray(ids_r, np.uint64)
    uv_l = np.asarray(uv_l, np.float32).reshape(-1, 2)
    uv_r = np.asarray(uv_r, np.float32).reshape(-1, 2)
    keep_l, keep_r = np.ones(len(ids_l), bool), np.ones(len(ids_r), bool)
    err_r = np.full(len(ids_r), np.nan)
    pos = np.searchsorted(ids_l, ids_r)
    paired = (pos < len(ids_l))
    paired[paired] = ids_l[pos[paired]] == ids_r[paired]
    jr, il = np.nonzero(paired)[0], pos[paired]
    dl, ok_l = bearings(uv_l[il], conv_l)
    dr, ok_r = bearings(uv_r[jr], conv_r)
    ok = ok_l & ok_r
    with np.errstate(invalid="ignore"):
        e = pair_error(E, dl, dr)
    e[~ok] = np.nan
    with np.errstate(invalid="ignore"):
        rej = ~(e <= max_error)     # NaN rejects
    err_r[jr] = e
    keep_r[jr[rej]] = False
    if mode == DROP_BOTH:
        keep_l[il[rej]] = False
    valid_e = e[ok]
    margin = float(np.min(np.abs(valid_e - max_error)) / max_error) if len(valid_e) else float("inf")
    return GateResult(keep_l, keep_r, err_r, int(paired.sum()), int(rej.sum()), int((~ok).sum()),
                      ids_r[jr[rej]], e[rej], margin)


def drop_both_lists(twin_l, twin_r, rejected_ids):
    """DROP_BOTH: the twin's lists (structured arrays with "id") minus the rejected ids."""
    rejected_ids = np.asarray(rejected_ids, np.uint64)
    return twin_l[~np.isin(twin_l["id"], rejected_ids)], twin_r[~np.isin(twin_r["id"], rejected_ids)]


@dataclass
class DropRight:
    """DROP_RIGHT against a never-gated twin: R(t) = R(t-1) + {ids of twin_right(t) outside R(t-1)
    that pair with the left list and are rejected at t}."""
    T: np.ndarray
    max_error: float
    conv_l: int = PLANE
    conv_r: int = PLANE
    removed: set = field(default_factory=set)

    def step(self, twin_l, uv_l, twin_r, uv_r):
        """(expected left list, expected right list, GateResult of this frame) from the twin's frame."""
        alive = ~np.isin(twin_r["id"], np.fromiter(self.removed, np.uint64, len(self.removed)))
        g = gate_lists(self.T, self.max_error, DROP_RIGHT, self.conv_l, self.conv_r, twin_l["id"], uv_l,
                       twin_r["id"][alive], np.asarray(uv_r)[alive])
        self.removed |= set(int(i) for i in g.rejected_ids)
        return twin_l, twin_r[alive][g.keep_r], g


# ------------------------------------------------------------------ the test sequences

def h3(right):
    """The right image with the rows of its right half rolled down by 3."""
    o = right.copy()
    w = o.shape[1]
    o[:, w // 2:] = np.roll(o[:, w // 2:], 3, axis=0)
    return o


def roll2(right):
    """The whole right image rolled down by 2."""
    return np.roll(right, 2, axis=0)


RIG_T = np.array([[1.0, 0, 0, 1.0], [0, 1.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])   # R = I, t = (1, 0, 0)
RIG_T_Y = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 1.0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])  # t = (0, 1, 0)
PINHOLE = (0, [120.0, 120.0, 80.0, 60.0, 0, 0, 0, 0, 0])
RADTAN = (0, [120.0, 120.0, 80.0, 60.0, -0.28, 0.07, 2e-4, 1.8e-5, 0.0])
EUCM = (1, [120.0, 120.0, 80.0, 60.0, 0.6, 1.1])
ONE_PIXEL = 1.0 / 120.0


def features(lst):
    """The oracle's [(id, x, y, aff)] as (ids u64, xy f32)."""
    ids = np.array([f[0] for f in lst], np.uint64)
    xy = np.array([[f[1], f[2]] for f in lst], np.float32).reshape(-1, 2)
    return ids, xy


def gated_oracle_run(O, frames, cam, convention=PLANE, T=RIG_T, max_error=ONE_PIXEL, w=160, h=120, levels=2,
                     grid=16):
    """The CPU oracle tracker under DROP_BOTH: per frame the reference gate on its lists (unprojected
    by the oracle's camera), then the oracle's remove_ids of the rejected.  Returns per frame
    (GateResult, ids_l before, ids_r before)."""
    trk = O.StereoTracker(w, h, levels, grid, 20, 0.01)
    c = O.camera(cam[0], cam[1], convention)
    out = []
    for left, right in frames:
        fl, fr = trk.process_frame(left, right)
        (il, xl), (ir, xr) = features(fl), features(fr)
        ul, ur = (O.unproject(c, xl)[0] if len(xl) else xl), (O.unproject(c, xr)[0] if len(xr) else xr)
        g = gate_lists(T, max_error, DROP_BOTH, convention, convention, il, ul, ir, ur)
        if g.n_rejected:
            trk.remove_ids(g.rejected_ids)
        out.append((g, il, ir))
    return out
