"""Inputs, case tables and one independent reference of the feature_tracker/ crate variant's edge
tests (test_ft_edges_cpu.py, test_ft_edges_gpu.py).

  tex / sequence / pair / checkerboard / black_band_pair    f32 images in [0, 1]
  select_corners(score, tracked_xy, threshold, min_dist)    add_points given a score map, brute force
  tracked_variants / border_ring / *_CASES                  the cases of each section

Everything is computed once per argument set and shared: treat every returned array as read-only.
select_corners restates feature_detection.rs:48-80 and :171-285 and the local_maxima rule that
oracle/ft_oracle.cpp and the comment above beats() in ft_detect.hip state; it searches no block
windows and sorts nothing before the O(n^2) comparison, so it shares no structure with either.
"""
from __future__ import annotations

import functools

import numpy as np

from tracker_shapes_reference import texture

f32 = np.float32
U32_MAX = (1 << 32) - 1


# ---------------------------------------------------------------------------------------------- inputs
def _ro(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, f32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def tex(h: int, w: int, seed: int) -> np.ndarray:
    """The multi-scale texture as f32 in [0, 1]; its mean is near 0.5 (LSSD divides by a patch mean)."""
    return _ro(texture(h, w, seed).astype(f32) / f32(255.0))


@functools.lru_cache(maxsize=None)
def sequence(h: int, w: int, k: int, seed: int) -> tuple:
    """k frames cut from one texture; the content of frame i is moved by (-2 i, +i) px against frame 0."""
    big = tex(h + k, w + 2 * k, seed)
    return tuple(_ro(big[(k - 1) - i:(k - 1) - i + h, 2 * i:2 * i + w]) for i in range(k))


def pair(h: int, w: int, seed: int) -> tuple:
    return sequence(h, w, 2, seed)


@functools.lru_cache(maxsize=None)
def checkerboard(h: int, w: int) -> np.ndarray:
    """8 px squares of 0.25 and 0.75: every gradient product and box sum is exact in f32, so the
    score map repeats the same few values all over the image (the tie fixture)."""
    y, x = np.mgrid[0:h, 0:w]
    return _ro(np.where(((x // 8) + (y // 8)) & 1, 0.75, 0.25))


TIE_SHAPE = (96, 128)   # (h, w)
TIE_BLURS = [0.5, 1.0, 2.0, 6.0]


@functools.lru_cache(maxsize=None)
def black_band_pair(h: int, w: int, seed: int) -> tuple:
    """pair() with columns [0, w / 3) exactly 0: with an unblurred pyramid a patch inside the band
    has mean 0 at level 0."""
    out = []
    for a in pair(h, w, seed):
        b = a.copy()
        b[:, :w // 3] = 0.0
        out.append(_ro(b))
    return tuple(out)


def band_points(h: int, w: int) -> np.ndarray:
    """A grid of centres over the whole image, 11 px apart; those with x < w / 3 - 8 see only zeros."""
    ys, xs = np.mgrid[9:h - 9:11, 9:w - 9:11]
    return np.ascontiguousarray(np.stack([xs.ravel(), ys.ravel()], 1).astype(f32) + f32(0.25))


def border_ring(h: int, w: int) -> np.ndarray:
    """Centres 0.3, 1.3, ... 9.3 px inside each of the four borders, two per distance and border:
    their 15 x 15 patterns lose the first lanes (top), the last (bottom) or interior ones (sides)."""
    pts = []
    for d in np.arange(10) + 0.3:
        for t in (1.0 / 3.0, 2.0 / 3.0):
            pts += [[d, t * (h - 1)], [w - 1 - d, t * (h - 1)], [t * (w - 1), d], [t * (w - 1), h - 1 - d]]
    return np.array(pts, f32)


# ------------------------------------------------------------------------- the selection reference
def round_sat_u32(v) -> int:
    """Rust's `f32::round() as u32`: half away from zero, then saturating (NaN and negatives -> 0)."""
    v = float(f32(v))
    if v != v or v <= 0.0:
        return 0
    if v >= 4294967296.0:
        return U32_MAX
    return min(int(np.floor(v + 0.5)), U32_MAX)   # exact in f64 for every f32 below 2^32


def nms_candidates(score: np.ndarray, threshold: float) -> list:
    """suppress_non_maximum(score, 1, threshold): per 2 x 2 block the greatest pixel, ties to the
    smaller (x, y); kept when >= threshold and nothing in the 3 x 3 ring around it outside the block
    is greater, or equal at a smaller (x, y).  Returns [(x, y, score)]."""
    h, w = score.shape
    thr = f32(threshold)
    out = []
    for y in range(0, h, 2):
        for x in range(0, w, 2):
            cells = [(cx, cy) for cy in range(y, min(h, y + 2)) for cx in range(x, min(w, x + 2))]
            top = max(score[cy, cx] for cx, cy in cells)
            if not top >= thr:
                continue
            bx, by = min(c for c in cells if score[c[1], c[0]] == top)
            ring = [(cx, cy) for cy in range(max(by - 1, 0), min(h, by + 2))
                    for cx in range(max(bx - 1, 0), min(w, bx + 2)) if (cx, cy) not in cells]
            if any(score[cy, cx] > top or (score[cy, cx] == top and (cx, cy) < (bx, by)) for cx, cy in ring):
                continue
            out.append((bx, by, top))
    return out


def select_corners(score: np.ndarray, tracked_xy, threshold: float, min_dist: int,
                   window_to_image_height: bool = False) -> np.ndarray:
    """add_points given the score map: k x 2 u32 (x, y) in (y, x) order.  window_to_image_height
    replaces local_maxima's `height` (the largest candidate y) by the image height: what a plain
    reading would expect, and NOT what the reference does; the CPU test uses it to show that the
    cases tell the two apart."""
    score = np.asarray(score, f32)
    h, w = score.shape
    md = int(min_dist)
    cand = [(x, y, s, False) for x, y, s in nms_candidates(score, threshold)]
    tr = np.zeros((0, 2), f32) if tracked_xy is None else np.asarray(tracked_xy, f32).reshape(-1, 2)
    if len(tr):
        top = f32(-np.inf)
        for c in cand:
            top = max(top, c[2])
        past = f32(top + f32(1.0))
        cand += [(round_sat_u32(p[0]), round_sat_u32(p[1]), past, True) for p in tr]
    if not cand:
        return np.zeros((0, 2), np.uint32)
    height = h if window_to_image_height else max(c[1] for c in cand)
    kept = []
    for cx, cy, cs, cpast in cand:
        lo, hi = cy - md, min(cy + md + 1, height)
        beaten = False
        for nx, ny, ns, _ in cand:
            if lo <= ny < hi and cx - md <= nx <= cx + md and (ns > cs or (ns == cs and (ny, nx) < (cy, cx))):
                beaten = True
                break
        if not beaten and not cpast and md <= cx < w - md and md <= cy < h - md:
            kept.append((cy, cx))
    kept.sort()
    return np.array([[x, y] for y, x in kept], np.uint32).reshape(-1, 2)


def equal_score_pairs(cand: list, min_dist: int) -> int:
    """Unordered pairs of NMS candidates with the same score and |dx|, |dy| <= min_dist."""
    c = np.array([(x, y) for x, y, _ in cand], np.int64).reshape(-1, 2)
    s = np.array([v for _, _, v in cand], f32)
    if len(c) < 2:
        return 0
    near = (np.abs(c[:, None, :] - c[None, :, :]).max(-1) <= min_dist) & (s[:, None] == s[None, :])
    return int((near.sum() - len(c)) // 2)


def threshold_value(score: np.ndarray, key) -> float:
    """'max': the greatest score (kept: the test is >=); 'above': the next f32 (nothing is kept)."""
    if key == "max":
        return float(score.max())
    if key == "above":
        return float(np.nextafter(f32(score.max()), f32(np.inf)))
    return float(key)


def tracked_variants(corners: np.ndarray, h: int, w: int) -> dict:
    """Tracked-feature lists built from a case's untracked corner list (k x 2 (x, y), k >= 4)."""
    c = np.asarray(corners, np.float64).reshape(-1, 2)
    ymin, ymax = c[:, 1].min(), c[:, 1].max()
    half = np.concatenate([c[0::3] + 0.5, c[1::3] - 0.5, c[2::3] + [0.5, -0.5]])
    span = np.stack([np.linspace(2.0, w - 3.0, 9), np.zeros(9)], 1)
    rng = np.random.default_rng(len(c))
    nonfinite = [[np.nan, 20.0], [20.0, np.nan], [np.nan, np.nan], [np.inf, 20.0], [20.0, np.inf], [-np.inf, 20.0],
                 [20.0, -np.inf], [1e10, 20.0], [20.0, 1e10], [-1e10, 20.0], [20.0, -1e10], [1e10, 1e10]]
    v = {
        "none": np.zeros((0, 2)),
        "one": c[len(c) // 2:len(c) // 2 + 1] + [1.0, 0.0],
        "on_corners": c[::2],
        "half_off": half,
        "below_all": span + [0.0, max(ymin - 1.0, 0.0)],     # rows at or above the first corner row
        "above_all": span + [0.0, min(ymax + 2.0, h - 1.0)],  # rows past the last corner row: moves `height`
        "outside": np.array([[-3.0, 5.0], [w + 4.0, 10.0], [10.0, h + 20.0], [-0.4, -0.4], [w - 0.5, h - 0.5]]),
        "nonfinite": np.array(nonfinite),
        "nonfinite_x_only": np.array([r for r in nonfinite if np.isfinite(r[1]) and abs(r[1]) < 1e9]),
        "many": np.concatenate([c + rng.uniform(-3.0, 3.0, c.shape) for _ in range(3)]),
    }
    return {k: np.ascontiguousarray(a, f32).reshape(-1, 2) for k, a in v.items()}


TRACKED_KEYS = ["none", "one", "on_corners", "half_off", "below_all", "above_all", "outside", "nonfinite",
                "nonfinite_x_only", "many"]

# (name, image, threshold key, min_dist, detection blur, tracked keys)
TEX_THR, TEX_MD, TEX_BLUR = 0.05, 2, 2.0
VARIANT_MD = 3   # cases with a larger min_dist build their tracked lists from the corners at this one


def _tie():
    return checkerboard(*TIE_SHAPE)


@functools.lru_cache(maxsize=None)
def selection_cases() -> tuple:
    """(name, image, threshold key, min_dist, detection blur, tracked-variant keys).  Tracked variants
    are built from the case's own untracked result; cases that have none name only 'none'."""
    cases = []
    for md in (0, 1, 3, 15):
        for thr in (0.0, 0.5, "max", "above"):
            keys = TRACKED_KEYS if thr == 0.5 else ["none"]
            cases.append((f"tie-md{md}-thr{thr}", _tie(), thr, md, 2.0, tuple(keys)))
    for blur in (0.5, 1.0, 6.0):
        cases.append((f"tie-blur{blur}", _tie(), 0.5, 3, blur, ("none", "on_corners", "above_all")))
    flat = _ro(np.full((40, 56), 0.5))
    cases.append(("flat-md0", flat, 0.0, 0, 2.0, ("none",)))
    cases.append(("flat-md3", flat, 0.0, 3, 2.0, ("none",)))
    for h, w in ((63, 65), (77, 129)):
        cases.append((f"tex-{w}x{h}", tex(h, w, 5), TEX_THR, TEX_MD, TEX_BLUR, tuple(TRACKED_KEYS)))
        cases.append((f"tex-{w}x{h}-md15", tex(h, w, 5), TEX_THR, 15, TEX_BLUR, ("none", "half_off", "above_all")))
    wide = tex(16, 2048, 6)
    cases.append(("wide-md7", wide, 0.02, 7, 1.0, ("none", "on_corners", "nonfinite")))
    cases.append(("wide-md0", wide, 0.02, 0, 1.0, ("none", "many")))
    return tuple(cases)


# ------------------------------------------------------------------------------------------ pyramid
# (h, w, levels, ratio)
PYRAMID_CASES = [
    (16, 16, 5, 2.0), (64, 64, 7, 2.0), (33, 40, 6, 2.0), (61, 97, 8, 1.5),
    (23, 17, 4, 1.0), (61, 97, 3, 1.0), (23, 17, 4, 1.02), (77, 131, 5, 1.3), (77, 131, 4, 3.0),
    (7, 63, 2, 2.0), (8, 64, 3, 2.0), (9, 65, 3, 2.0), (17, 127, 3, 2.0), (7, 128, 2, 2.0), (8, 129, 3, 2.0),
    (9, 63, 3, 1.5), (17, 64, 4, 2.0),
]
PYRAMID_SIGMAS = [0.0, -1.0, 0.5, 5.0]
PYRAMID_SIGMA_SHAPES = [(33, 40, 3, 2.0), (17, 129, 2, 2.0)]
COPY_DIMS = {(23, 17, 4, 1.0): [(17, 23)] * 4,
             (61, 97, 3, 1.0): [(97, 61)] * 3,
             (23, 17, 4, 1.02): [(17, 23), (17, 23), (16, 22), (16, 22)]}
# (h, w, levels, ratio) that build_image_pyramid refuses on the host
PYRAMID_REFUSED = [(16, 16, 0, 2.0), (16, 16, 9, 2.0), (16, 16, 7, 2.0), (16, 3, 1, 2.0), (3, 16, 1, 2.0),
                   (16, 16, 2, 0.0), (16, 16, 2, -2.0)]


def noise(h: int, w: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed * 7919 + h * 131 + w).uniform(0.0, 1.0, (h, w)).astype(f32)


# unblurred pyramids of an image that is not in [0, 1]: level 0 is the image as it came, a same-size
# level is a copy of it (image's resize returns one), and only a real resize clamps and drops -0
UNCLAMPED_CASES = [(23, 17, 4, 1.0), (23, 17, 4, 1.02), (33, 40, 3, 2.0)]


def unclamped(h: int, w: int) -> np.ndarray:
    """Values in [-0.5, 1.5), every seventh pixel -0.0."""
    img = noise(h, w, 5) * f32(2.0) - f32(0.5)
    img.ravel()[::7] = f32(-0.0)
    return img


# -------------------------------------------------------------------------------------------- score
SCORE_BLURS = [0.5, 32.0, 64.0]
SCORE_BOXES = {0.5: [1, 1, 1], 32.0: [63, 63, 65], 64.0: [127, 127, 129]}
SCORE_SHAPES = [(16, 16), (65, 63), (64, 64), (63, 65), (192, 128), (200, 129), (129, 200), (2048, 16), (16, 2048)]


# ----------------------------------------------------------------------------------------------- LK
# (h, w, levels, ratio, SSD tracks, LSSD tracks): "tracks" = >= 20 valid and >= 10 invalid on the oracle
LK_CASES = [
    (120, 160, 3, 2.0, True, True),
    (77, 131, 1, 2.0, True, True),
    (77, 131, 3, 1.0, True, True),
    (77, 131, 5, 1.3, True, True),
    (61, 97, 4, 2.0, True, False),     # level 3 is 12 x 8: every lane misses; LSSD divides 0 by 0 there
]
# (h, w, levels): no LSSD track survives -- every lane misses at the top levels (0 / 0), or the
# image is as small as the pattern.  SSD keeps H = lambda I there and a few centres survive.
LK_ALL_FAIL = [(33, 40, 6), (64, 64, 7), (16, 16, 1)]
LK_ITERS = [0, 1, 2, 25]
LK_LAMBDAS = [0.0, 1e-6, 100.0, 1e6]
LK_PARAM_SHAPE = (77, 131, 3, 2.0)
BAND_SHAPE = (120, 160, 3)             # (h, w, levels), unblurred pyramid
LK_SEED = 21


def lk_bad_points(h: int, w: int) -> np.ndarray:
    """NaN, infinite, negative and far positions: each must come back invalid with the identity."""
    return np.array([[np.nan, 10.0], [10.0, np.nan], [np.inf, 10.0], [10.0, -np.inf], [-1.0, 10.0], [10.0, -0.6],
                     [-1e10, -1e10], [1e10, 10.0], [w + 0.0, h / 2], [w / 2, h + 0.0]], f32)


# ------------------------------------------------------------------------------------------- handle
# (h, w, levels, ratio, preprocessing blur)
HANDLE_CASES = [(61, 97, 4, 2.0, True), (77, 131, 5, 1.3, True), (64, 64, 1, 2.0, True), (77, 131, 3, 1.0, True),
                (61, 97, 3, 2.0, False)]
HANDLE_FRAMES = 4
HANDLE_SEED = 31
# the smallest of a few shapes tried whose frame 0 has > 1024 features and frame 1 > 1024 tracked ones
DENSE_CASE = dict(h=184, w=272, nlevels=3, threshold=0.01, min_dist=1, detection_blur=1.0)


def handle_config(mod, nlevels=3, ratio=2.0, blur=True, **kw):
    """A FeatureTrackingConfig (rsvio.ft) or ft_config (the oracle) with the texture's detection settings."""
    args = dict(nlevels=nlevels, ratio=ratio, preprocessing_blur=blur, detection_threshold=TEX_THR,
                detection_min_dist=TEX_MD, detection_blur=TEX_BLUR)
    args.update(kw)
    make = getattr(mod, "FeatureTrackingConfig", None) or mod.ft_config
    return make(**args)


DYING_CASE = (61, 97, 3, 2.0)   # (h, w, levels, ratio)


@functools.lru_cache(maxsize=None)
def dying_sequence() -> tuple:
    """Frames 0, 1 of one texture, then uniform noise, then frame 0 again: the oracle keeps tracks
    from frame 0 to 1 and none into the noise (test_ft_edges_cpu.py)."""
    h, w = DYING_CASE[:2]
    a = sequence(h, w, 2, HANDLE_SEED)
    return a[0], a[1], _ro(np.random.default_rng(1).uniform(0.0, 1.0, (h, w))), a[0]
