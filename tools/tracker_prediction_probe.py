"""What a motion-predicted frame costs, and whether a handle without a prediction is as fast as before.

Workload: config 2's frame (752 x 480, L = 3, grid 30, about 415 features per camera) with cameras
attached (pinhole f = 460), device-resident images, one handle.  Per build and setting:
  device_ms   HIP events on the handle's stream around rsvio_tracker_submit_device (the frame's
              launches and its read-back copies)
  wall_ms     a host clock around rsvio_tracker_process_frame_device (it ends in a host wait); for
              "predicted" the rsvio_tracker_set_prediction call before it is inside the clock
Settings: "off" (no prediction) and "predicted" (a hint of 0.2 degrees of yaw set before every frame,
so every feature is seeded a pixel or two from its position and the tracks converge as before);
builds: this tree's library and, with --parent-lib, another build of the library (the parent
commit's), which only knows "off".  The driver starts one worker process per build and round and
alternates the builds (--rounds, each worker --reps timed frames after --warmup); inside a worker the
settings alternate frame by frame, each on a handle of its own, and each handle alternates the two
ways of running a frame.  Samples are pooled over the rounds: median, p10, p90.
`unpredicted_level_with_parent` says whether the p10-p90 ranges of "off" overlap between the builds.

usage: python tools/tracker_prediction_probe.py [--parent-lib FILE] [--rounds 3] [--reps 40] [--frames-file NPY]
                                                [--out profiles/tracker_prediction_probe.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "rs-vio_amd")]

import numpy as np  # noqa: E402

W, H, LEVELS, GRID, MAX_IT, THRESH = 752, 480, 3, 30, 20, 0.01
SEQ = [0, 1, 2, 3, 2, 1]
FOCAL = 460.0
YAW_DEG = 0.2


def render(path):
    from rsvio import synthetic as S
    np.save(path, np.stack([np.stack(f) for f in S.stereo_sequence(4, W, H)]))


def worker(a):
    import torch

    import rsvio
    from rsvio import _lib
    from rsvio._lib import ptr
    from rsvio.camera import Camera
    lib = _lib.load()
    rsvio.require_device(0)
    has_pred = hasattr(lib, "rsvio_tracker_set_prediction")
    settings = ["off"] + (["predicted"] if has_pred else [])
    cam = Camera.opencv5(FOCAL, FOCAL, W / 2.0, H / 2.0)
    imgs = torch.from_numpy(np.load(a.frames_file)).cuda()            # F x 2 x H x W
    torch.cuda.synchronize()
    c, s = math.cos(math.radians(YAW_DEG)), math.sin(math.radians(YAW_DEG))
    pred = None
    if has_pred:
        pred = _lib.TrackPrediction()
        pred.R_l[:] = pred.R_r[:] = [c, 0.0, -s, 0.0, 1.0, 0.0, s, 0.0, c]
    legs = {}
    for name in settings:
        t = rsvio.StereoPatchTracker(W, H, levels=LEVELS, grid_size=GRID, optical_flow_max_iterations=MAX_IT,
                                     optical_flow_convergence_threshold=THRESH)
        t.set_cameras(cam, cam)
        ext = torch.cuda.ExternalStream(lib.rsvio_tracker_stream(t._h))
        legs[name] = dict(t=t, ext=ext, dev=[], wall=[], feats=[], seeded=[])
    nl, nr = C.c_size_t(0), C.c_size_t(0)
    for k in range(2 * (a.warmup + a.reps)):
        f = SEQ[k % len(SEQ)]
        dl, dr = imgs[f, 0].data_ptr(), imgs[f, 1].data_ptr()
        timed = k >= 2 * a.warmup
        for name in settings:
            g = legs[name]
            t = g["t"]
            if k % 2 == 0:   # wall: the blocking call
                t0 = time.perf_counter()
                if name == "predicted":
                    _lib.check(lib.rsvio_tracker_set_prediction(t._h, C.byref(pred)))
                _lib.check(lib.rsvio_tracker_process_frame_device(t._h, dl, dr, ptr(t._out_l), t.cap, C.byref(nl),
                                                                  ptr(t._out_r), t.cap, C.byref(nr)))
                if timed:
                    g["wall"].append((time.perf_counter() - t0) * 1e3)
            else:            # device: events around the enqueue
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if name == "predicted":
                    _lib.check(lib.rsvio_tracker_set_prediction(t._h, C.byref(pred)))
                e0.record(g["ext"])
                _lib.check(lib.rsvio_tracker_submit_device(t._h, dl, dr))
                e1.record(g["ext"])
                _lib.check(lib.rsvio_tracker_collect(t._h, ptr(t._out_l), t.cap, C.byref(nl), ptr(t._out_r), t.cap,
                                                     C.byref(nr)))
                e1.synchronize()
                if timed:
                    g["dev"].append(e0.elapsed_time(e1))
            if timed:
                g["feats"].append(float(nl.value))
                if name == "predicted":
                    g["seeded"].append(float(t.prediction_counts().n_seeded[0]))
    out = {}
    for name in settings:
        g = legs[name]
        out[name] = dict(device_ms=g["dev"], wall_ms=g["wall"], features_left=float(np.median(g["feats"])),
                         seeded_left=float(np.median(g["seeded"])) if g["seeded"] else 0.0)
        g["t"].close()
    print("PROBE " + json.dumps(out), flush=True)


def _stats(x):
    x = np.asarray(x, np.float64)
    return dict(median=float(np.median(x)), p10=float(np.percentile(x, 10)), p90=float(np.percentile(x, 90)),
                n=int(len(x)))


def driver(a):
    tmp = None
    if not a.frames_file:
        tmp = tempfile.NamedTemporaryFile(suffix=".npy", delete=False)
        tmp.close()
        render(tmp.name)
        a.frames_file = tmp.name
    builds = ([("parent", a.parent_lib)] if a.parent_lib else []) + [("tree", None)]
    pooled = {}
    for rnd in range(a.rounds):
        for build, libpath in builds:
            env = dict(os.environ)
            if libpath:
                env["RSVIO_LIB"] = str(Path(libpath).resolve())
            else:
                env.pop("RSVIO_LIB", None)
            p = subprocess.run([sys.executable, __file__, "--worker", "--frames-file", a.frames_file, "--reps",
                                str(a.reps), "--warmup", str(a.warmup)], env=env, capture_output=True, text=True,
                               timeout=600)
            if p.returncode != 0:   # a failed worker ends the probe: nothing more is started
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"worker ({build}, round {rnd}) failed with {p.returncode}")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("PROBE ")][-1]
            for key, v in json.loads(line[6:]).items():
                d = pooled.setdefault(f"{build}/{key}", dict(device_ms=[], wall_ms=[], info={}))
                d["device_ms"] += v["device_ms"]
                d["wall_ms"] += v["wall_ms"]
                d["info"] = dict(features_left=v["features_left"], seeded_left=v["seeded_left"])
            print(f"round {rnd} {build} done", flush=True)
    if tmp:
        os.unlink(tmp.name)
    rows = []
    for key, d in pooled.items():
        build, setting = key.split("/")
        row = dict(build=build, setting=setting, **d["info"], device_ms=_stats(d["device_ms"]),
                   wall_ms=_stats(d["wall_ms"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(shape=[W, H], levels=LEVELS, grid=GRID, focal=FOCAL, yaw_deg=YAW_DEG, rounds=a.rounds,
               reps_per_round=a.reps, rows=rows)
    by = {(r["build"], r["setting"]): r for r in rows}
    if a.parent_lib:
        lvl = {}
        for m in ("device_ms", "wall_ms"):
            p, t = by["parent", "off"][m], by["tree", "off"][m]
            lvl[m] = bool(p["p10"] <= t["p90"] and t["p10"] <= p["p90"])
        res["unpredicted_level_with_parent"] = lvl
    res["prediction_cost_us_per_frame"] = {
        m: (by["tree", "predicted"][m]["median"] - by["tree", "off"][m]["median"]) * 1e3 for m in ("device_ms", "wall_ms")}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--frames-file", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tracker_prediction_probe.json"))
    a = ap.parse_args()
    if a.reps < 30:
        ap.error("--reps must be at least 30")
    if a.worker:
        worker(a)
    else:
        driver(a)


if __name__ == "__main__":
    main()
