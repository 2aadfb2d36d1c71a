"""Inputs and case tables of the tracker shape tests (test_tracker_shapes_cpu.py, test_tracker_shapes_gpu.py).

  texture(h, w, seed)                     u8 image with gradient at every scale from 4 to 256 px
  shifted_frames(h, w, k, seed, noise)    k stereo pairs cut from one texture, moved frame by frame
  pyramid_plan(w, h, levels)              PyramidPlan::init (pyramid.hip) restated in numpy f32
  *_CASES / lk_* / fast_* / pipeline_*    the shapes and parameters of each section, and their inputs

Everything is computed once per argument set and shared: treat every returned array as read-only.
The references themselves come from the CPU oracle (oracle/) in the test files.
"""
from __future__ import annotations

import functools

import numpy as np

f32 = np.float32


# ---------------------------------------------------------------------------------------------- inputs
def _upsample(grid: np.ndarray, h: int, w: int, cell: int) -> np.ndarray:
    """Bilinear up-sampling of a grid with `cell` pixels between its nodes, as two small products."""
    def weights(n, m):
        pos = np.arange(n, dtype=np.float64) / cell
        i0 = np.floor(pos).astype(np.int64)
        fr = pos - i0
        W = np.zeros((n, m))
        W[np.arange(n), i0] = 1.0 - fr
        W[np.arange(n), i0 + 1] += fr
        return W
    return weights(h, grid.shape[0]) @ grid @ weights(w, grid.shape[1]).T


@functools.lru_cache(maxsize=None)
def texture(h: int, w: int, seed: int) -> np.ndarray:
    """Sum of bilinearly up-sampled uniform random grids with cell sizes 4 .. 256 (the two finest
    counted twice, for FAST corners in most 8 px cells), normalised to 0..255: every pyramid level
    down to level 7 (one pixel per 128) keeps some gradient."""
    rng = np.random.default_rng(seed)
    acc = np.zeros((h, w))
    for cell, weight in ((4, 2.0), (8, 2.0), (16, 1.0), (32, 1.0), (64, 1.0), (128, 1.0), (256, 1.0)):
        grid = rng.uniform(0.0, 1.0, (h // cell + 2, w // cell + 2))
        acc += weight * _upsample(grid, h, w, cell)
    acc -= acc.min()
    img = np.round(acc * (255.0 / acc.max())).astype(np.uint8)
    img.setflags(write=False)
    return img


def _noisy(img: np.ndarray, rng, noise: int) -> np.ndarray:
    if noise <= 0:
        return np.ascontiguousarray(img)
    n = rng.integers(-noise, noise + 1, img.shape)
    return np.clip(img.astype(np.int64) + n, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def shifted_frames(h: int, w: int, k: int, seed: int, noise: int = 0):
    """k stereo pairs (left, right) cut from one texture.  The content of frame i is moved by
    (-2 i, +i) px against frame 0, the right image by another -4 px in x (a 4 px disparity);
    every image gets its own uniform integer noise of +-noise grey levels."""
    big = texture(h + k, w + 2 * k + 4, seed)
    rng = np.random.default_rng(seed + 7919)
    out = []
    for i in range(k):
        y0, x0 = (k - 1) - i, 2 * i
        left = _noisy(big[y0:y0 + h, x0:x0 + w], rng, noise)
        right = _noisy(big[y0:y0 + h, x0 + 4:x0 + 4 + w], rng, noise)
        for a in (left, right):
            a.setflags(write=False)
        out.append((left, right))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def shifted_pair(h: int, w: int, seed: int, noise: int = 0):
    """Two images of one texture, the second's content moved by (-2, +3) px."""
    big = texture(h + 3, w + 2, seed)
    rng = np.random.default_rng(seed + 104729)
    a = _noisy(big[3:3 + h, 0:w], rng, noise)
    b = _noisy(big[0:h, 2:2 + w], rng, noise)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def identity_states(xy) -> np.ndarray:
    xy = np.asarray(xy, f32).reshape(-1, 2)
    aff = np.zeros((len(xy), 6), f32)
    aff[:, 0] = aff[:, 3] = 1.0
    aff[:, 4:6] = xy
    return aff


def outside_states(h: int, w: int) -> np.ndarray:
    """8 positions outside the image or inside its 2 px border."""
    return np.array([[-5.0, h / 2], [w + 3.0, h / 2], [w / 2, -1.0], [w / 2, h + 10.0], [0.5, 0.5],
                     [w - 1.2, h / 2], [w / 2, 1.4], [1e9, 5.0]], f32)


@functools.lru_cache(maxsize=None)
def lk_states(h: int, w: int, n: int, seed: int) -> np.ndarray:
    """n identity Affine2 states: n - 8 at random positions of the image, then outside_states."""
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(0.0, w - 1.0, n - 8), rng.uniform(0.0, h - 1.0, n - 8)], 1)
    aff = identity_states(np.concatenate([xy.astype(f32), outside_states(h, w)]))
    aff.setflags(write=False)
    return aff


def lk_seeds(aff: np.ndarray, shift) -> np.ndarray:
    """One seed per state: entry 3j the exact displaced position, 3j + 1 that plus (1.5, -1.5) px,
    3j + 2 NaN ("the own position")."""
    seeds = aff[:, 4:6] + np.asarray(shift, f32)
    seeds[1::3] += np.array([1.5, -1.5], f32)
    seeds[2::3] = np.nan
    return seeds.astype(f32)


# ------------------------------------------------------------------------------------- pyramid plan
TW, TH, STRIP_COLS, LDS_CAP = 64, 8, 320, 64 << 10


def taps(in_len: int, out_len: int):
    """(left, count) of every output index: make_taps_kernel's f32 arithmetic (image 0.25 sample.rs)."""
    o = np.arange(out_len, dtype=f32)
    ratio = f32(in_len) / f32(out_len)
    support = f32(max(ratio, f32(1.0)))
    inputc = (o + f32(0.5)) * ratio
    left = np.clip(np.floor(inputc - support).astype(np.int64), 0, in_len - 1)
    right = np.minimum(np.maximum(np.ceil(inputc + support).astype(np.int64), left + 1), in_len)
    return left, right - left


@functools.lru_cache(maxsize=None)
def pyramid_plan(w: int, h: int, levels: int) -> dict:
    """tile_w, tile_h (8 entries, zero where unused), direct mask, lds_bytes and per level the largest
    (strip, vert) footprint in bytes, as PyramidPlan::init computes them."""
    tile_w, tile_h, foot = [0] * 8, [0] * 8, {}
    direct, lds = 0, 0
    for i in range(1, levels):
        nw, nh = w >> i, h >> i
        rx, ry = f32(w) / f32(nw), f32(h) / f32(nh)
        tile_h[i] = max(1, min(TH, int(f32(16.0) / ry)))
        tile_w[i] = max(1, min(TW, int(np.floor((f32(STRIP_COLS) - f32(2.0) * rx - f32(4.0)) / rx))))
        xl_, xc_ = taps(w, nw)
        yl_, yc_ = taps(h, nh)
        strip = vert = 0
        for ox0 in range(0, nw, tile_w[i]):
            ox1 = min(ox0 + tile_w[i], nw)
            xl, xr = int(xl_[ox0]), int(xl_[ox1 - 1] + xc_[ox1 - 1])
            pd = (xr - (xl & ~3) + 3) // 4
            for oy0 in range(0, nh, tile_h[i]):
                oy1 = min(oy0 + tile_h[i], nh)
                yl, yr = int(yl_[oy0]), int(yl_[oy1 - 1] + yc_[oy1 - 1])
                strip = max(strip, 4 * pd * (yr - yl))
                vert = max(vert, 4 * (oy1 - oy0) * (xr - xl))
        foot[i] = (strip, vert)
        if strip + vert > LDS_CAP:
            direct |= 1 << i
            lds = max(lds, vert)
        else:
            lds = max(lds, strip + vert)
    return {"tile_w": tile_w, "tile_h": tile_h, "direct": direct, "lds_bytes": lds, "foot": foot}


# (h, w, levels, the direct mask the issue expects -- None where it names none)
PYRAMID_CASES = [
    (256, 256, 8, 0),
    (400, 416, 8, 1 << 7),
    (600, 1000, 8, 1 << 7),
    (383, 447, 7, 0),
    (130, 200, 7, 0),
    (61, 97, 1, None),
    (61, 97, 4, None),
    (61, 97, 5, None),
    (33, 40, 1, None),
]
# the shapes of PYRAMID_CASES whose level 7 reads its vertical taps from HBM: one texture image each
DIRECT_SHAPES = [(400, 416), (600, 1000)]
# rsvio_build_pyramids_d, packed: (n images, h, w, levels)
PACKED_CASES = [(3, 61, 97, 3), (3, 33, 40, 2)]
OFFSET_CASE = (2, 120, 160, 3)   # with the source base offset by 4 B / the destination base by 1 B


def noise_image(h: int, w: int, levels: int, k: int = 0) -> np.ndarray:
    return np.random.default_rng(h * 1000 + levels + 77 * k).integers(0, 256, (h, w), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- LK
DEPTH_SHAPE = (1664, 1920)
DEPTH_SHIFT = (-2.0, 3.0)
# (h, w, levels): pyramids whose top level is 1 x 1, 3 x 3 or 5 x 6 -- too small for any template
UNDERSIZED_CASES = [(20, 20, 5), (16, 24, 5), (40, 48, 4), (80, 96, 5), (400, 416, 8)]
MIXED_CASE = (33, 40, 2)
EDGE_SHAPE = (208, 240, 3)
EDGE_THRESH = [0.0, 1e-45, float(np.finfo(f32).tiny), 1e-30, 1e-3, 0.5, 5.0, 1e6, 3e38, float("inf"), float("nan"), -1.0]
EDGE_ITERS = [0, 1, 2, 3, 5, 100]
EDGE_COMBOS = list(dict.fromkeys([(it, th) for th in EDGE_THRESH for it in (3, 20)] +
                                 [(it, th) for it in EDGE_ITERS for th in (0.01, 0.5)]))
EDGE_SAME_AS_DEFAULT = {(20, 0.01), (100, 0.01)}   # may equal the default outputs


def edge_pair():
    """The 208 x 240 pair of the parameter-edge tests: frames 0 and 4 of a noisy sequence (content
    moved by (-8, +4) px), so that the default parameters need more than five iterations at some
    level on most states."""
    h, w, _ = EDGE_SHAPE
    fr = shifted_frames(h, w, 5, 41, 6)
    return fr[0][0], fr[4][0]


# -------------------------------------------------------------------------------------------- FAST
FAST_CASES = [(120, 160, 8), (61, 97, 16), (128, 128, 128), (150, 200, 37), (120, 160, 40), (64, 64, 9),
              (45, 50, 45), (38, 38, 8), (40, 300, 13), (280, 328, 8)]
FAST_EMPTY = (38, 38, 8)


@functools.lru_cache(maxsize=None)
def fast_image(h: int, w: int, g: int) -> np.ndarray:
    img = _noisy(texture(h, w, 500 + g), np.random.default_rng(h * 7 + w * 3 + g), 40)
    img.setflags(write=False)
    return img


def fast_existing(h: int, w: int, g: int, found_xy: np.ndarray) -> np.ndarray:
    """Existing points: every second found corner + 0.5; the roundf bin edges of the first and last
    grid line in x and in y; a negative, a huge and a NaN coordinate."""
    xs, ys = (w % g) // 2, (h % g) // 2
    ex = [xs + k * g + d for k in (0, w // g) for d in (-0.5, 0.5)]
    ey = [ys + k * g + d for k in (0, h // g) for d in (-0.5, 0.5)]
    edges = [[x, h / 2] for x in ex] + [[w / 2, y] for y in ey] + [[x, y] for x in ex for y in ey]
    parts = [found_xy[::2].astype(f32) + f32(0.5), np.array(edges, f32),
             np.array([[-3, 5], [1e9, 5], [np.nan, 5]], f32)]
    return np.ascontiguousarray(np.concatenate([p.reshape(-1, 2) for p in parts]).astype(f32))


# ---------------------------------------------------------------------------------------- pipeline
# (h, w, levels, grid, noise, frames): noise raised until the oracle loses an id within the frames
PIPELINE_CASES = [
    (208, 240, 5, 37, 24, 3),
    (120, 160, 1, 16, 16, 3),
    (61, 97, 3, 9, 16, 3),
    (280, 328, 3, 8, 10, 4),
    (832, 960, 7, 100, 24, 3),
    (1664, 1920, 8, 128, 12, 3),
]
MANY_CELLS = (280, 328, 3, 8)   # 41 x 35 = 1435 cells; its lists pass 1024 entries
BATCH_CASE = (61, 97, 3, 9)


def pipeline_frames(h, w, levels, grid, noise, k):
    return shifted_frames(h, w, k, 1000 + h + levels, noise)
