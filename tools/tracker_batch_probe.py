"""Batched process_frame against n sequential single-stream calls.

Config 2's shape (752 x 480, L = 3, grid 30: 400 cells, about 415 features per camera); stream s sees the
config-2 sequence translated by (s % 8, s // 8) px, as bench.py's measure_tracker_batched_row;
images are device-resident.  For n in --n (default 1 8 64) streams, every timed frame runs
  (a) n rsvio_tracker_process_frame_device calls in a loop (three launches and one host wait each), and
  (b) one rsvio_tracker_batch_process_frames over n other handles fed the same images (one upload
      of the tables, three launches, one read-back, one wait),
alternating inside each frame in one process, both on the C ABI with their arguments marshalled
beforehand.  Reported per n: the median and minimum of the wall time per call (a host clock around
calls that end in a host wait) for both legs, of (b)'s device_ms (its three launches by HIP events),
the same per frame, and beside them the stateless ceiling: rows.tracker_batched's pyramid + LK time
for n streams (measure_tracker_batched_row: the primitives alone, no FAST, no append / pack, no
read-back).  (b)'s lists are checked against (a)'s, byte for byte, on every frame.

usage: python tools/tracker_batch_probe.py [--n 1 8 64] [--frames 60] [--out FILE]   (default: profiles/tracker_batch_probe.json)
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "rs-vio_amd")]

import numpy as np  # noqa: E402

import bench  # noqa: E402
import rsvio  # noqa: E402
from rsvio import _lib  # noqa: E402
from rsvio._lib import ptr  # noqa: E402

GRID = 30


def _stats(x):
    x = np.asarray(x, np.float64)
    return dict(median=float(np.median(x)), min=float(np.min(x)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tracker_batch_probe.json"))
    a = ap.parse_args()
    if a.frames < 50:
        ap.error("--frames must be at least 50")
    import torch
    lib = _lib.load()
    rsvio.require_device(0)
    trk = bench.TrackerWorkload(0)
    n_max = max(a.n)
    seq = trk.seq
    imgs = torch.empty((len(set(seq)), n_max, 2, bench.H, bench.W), dtype=torch.uint8, device=trk.imgs.device)
    for s in range(n_max):
        imgs[:, s] = torch.roll(trk.imgs, shifts=(s // 8, s % 8), dims=(-2, -1))
    torch.cuda.synchronize()
    rows = []
    for n in a.n:
        def make():
            return [rsvio.StereoPatchTracker(bench.W, bench.H, levels=bench.LEVELS, grid_size=GRID,
                                             optical_flow_max_iterations=bench.MAX_IT,
                                             optical_flow_convergence_threshold=bench.THRESH) for _ in range(n)]
        single, batched = make(), make()
        tb = rsvio.TrackerBatch(batched)
        nl = [(C.c_size_t(0), C.c_size_t(0)) for _ in range(n)]
        calls, tabs = {}, {}
        for t in set(seq):   # both legs' arguments, per frame of the cycle
            calls[t] = [(tr._h, imgs[t, s, 0].data_ptr(), imgs[t, s, 1].data_ptr(), ptr(tr._out_l), tr.cap,
                         C.byref(nl[s][0]), ptr(tr._out_r), tr.cap, C.byref(nl[s][1]))
                        for s, tr in enumerate(single)]
            tabs[t] = tb._frames([imgs[t, s, 0] for s in range(n)], [imgs[t, s, 1] for s in range(n)])
        ms = C.c_double(0.0)
        wall = {"single": [], "batch": []}
        dev, feats = [], []
        for k in range(a.warmup + a.frames):
            t = seq[k % len(seq)]
            t0 = time.perf_counter()
            for c in calls[t]:
                _lib.check(lib.rsvio_tracker_process_frame_device(*c))
            t1 = time.perf_counter()
            _lib.check(lib.rsvio_tracker_batch_process_frames(tb._h, C.addressof(tabs[t][0]), C.byref(ms)))
            t2 = time.perf_counter()
            for s in range(n):   # (b) returns (a)'s lists
                c = tabs[t][0][s]
                assert (c.status, c.n_l, c.n_r) == (0, nl[s][0].value, nl[s][1].value), (k, s)
                assert np.array_equal(batched[s]._out_l[:c.n_l].view(np.uint8), single[s]._out_l[:c.n_l].view(np.uint8))
                assert np.array_equal(batched[s]._out_r[:c.n_r].view(np.uint8), single[s]._out_r[:c.n_r].view(np.uint8))
            if k < a.warmup:
                continue
            wall["single"].append((t1 - t0) * 1e3)
            wall["batch"].append((t2 - t1) * 1e3)
            dev.append(ms.value)
            feats.append(float(np.mean([v[0].value for v in nl])))
        tb.close()
        for tr in single + batched:
            tr.close()
        ceil = bench.measure_tracker_batched_row(trk, 0, n_streams=n)
        row = dict(n=n, frames=a.frames, shape=[bench.W, bench.H], levels=bench.LEVELS, grid=GRID,
                   features_per_camera=float(np.median(feats)),
                   single_wall_ms=_stats(wall["single"]), batch_wall_ms=_stats(wall["batch"]),
                   batch_device_ms=_stats(dev),
                   per_frame_us=dict(single_wall=float(np.median(wall["single"])) / n * 1e3,
                                     batch_wall=float(np.median(wall["batch"])) / n * 1e3,
                                     batch_device=float(np.median(dev)) / n * 1e3,
                                     stateless_pyramid_lk=(ceil["pyramid_ms"] + ceil["lk_ms"]) / n * 1e3),
                   stateless=dict(pyramid_ms=ceil["pyramid_ms"], lk_ms=ceil["lk_ms"], ms_per_step=ceil["ms_per_step"]),
                   wall_gain=float(np.median(wall["single"]) / np.median(wall["batch"])))
        rows.append(row)
        print(json.dumps(row), flush=True)
    trk.close()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
