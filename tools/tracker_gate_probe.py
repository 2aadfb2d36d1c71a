"""What the tracker's stereo gate costs per frame, and whether a handle without one is as fast as before.

Workload: config 2's frame (752 x 480, L = 3, grid 30, about 415 features per camera) with cameras
attached (pinhole f = 460; rig R = I, t = (1, 0, 0), the geometry of the synthetic stereo pair;
max_error one pixel), device-resident images; stream s of a batch sees the sequence translated by
(s % 8, s // 8) px as tools/tracker_batch_probe.py.  Per build and setting, for n = 1 and n = 64
handles:
  device_ms   rsvio_tracker_batch_process_frames' own HIP events around its three launches
  wall_ms     a host clock around that call (it ends in a host wait), and for n = 1 also around
              rsvio_tracker_process_frame_device
Settings: "off" (no gate), "drop_right", "drop_both"; builds: this tree's library and, with
--parent-lib, another build of the library (the parent commit's), which only knows "off".  The
driver starts one worker process per build and round and alternates the builds (--rounds, each
worker --reps timed frames after --warmup); inside a worker the settings alternate frame by frame.
Samples are pooled over the rounds: median, p10, p90.  `gate_off_level_with_parent` says whether
the p10-p90 ranges of "off" overlap between the two builds.

usage: python tools/tracker_gate_probe.py [--parent-lib FILE] [--rounds 3] [--reps 40] [--frames-file NPY]
                                          [--out profiles/tracker_stereo_gate_probe.json]
"""
import argparse
import ctypes as C
import json
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
RIG = np.array([[1.0, 0, 0, 1.0], [0, 1.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])


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
    has_gate = hasattr(lib, "rsvio_tracker_set_stereo_gate")
    settings = ["off"] + (["drop_right", "drop_both"] if has_gate else [])
    cam = Camera.opencv5(FOCAL, FOCAL, W / 2.0, H / 2.0)
    base = torch.from_numpy(np.load(a.frames_file)).cuda()            # F x 2 x H x W
    out = {}
    for n in (1, 64):
        imgs = torch.empty((base.shape[0], n, 2, H, W), dtype=torch.uint8, device=base.device)
        for s in range(n):
            imgs[:, s] = torch.roll(base, shifts=(s // 8, s % 8), dims=(-2, -1))
        torch.cuda.synchronize()
        legs = {}
        for name in settings:
            ts = [rsvio.StereoPatchTracker(W, H, levels=LEVELS, grid_size=GRID, optical_flow_max_iterations=MAX_IT,
                                           optical_flow_convergence_threshold=THRESH) for _ in range(n)]
            single = rsvio.StereoPatchTracker(W, H, levels=LEVELS, grid_size=GRID, optical_flow_max_iterations=MAX_IT,
                                              optical_flow_convergence_threshold=THRESH) if n == 1 else None
            for t in ts + ([single] if single else []):
                t.set_cameras(cam, cam)
                if name != "off":
                    t.set_stereo_gate(rsvio.StereoGate(name, 1.0 / FOCAL, RIG))
            tb = rsvio.TrackerBatch(ts)
            tabs = {f: tb._frames([imgs[f, s, 0] for s in range(n)], [imgs[f, s, 1] for s in range(n)]) for f in set(SEQ)}
            legs[name] = dict(ts=ts, tb=tb, tabs=tabs, single=single, dev=[], wall=[], wall_single=[], feats=[], rej=[])
        ms, nl, nr = C.c_double(0.0), C.c_size_t(0), C.c_size_t(0)
        for k in range(a.warmup + a.reps):
            f = SEQ[k % len(SEQ)]
            for name in settings:
                g = legs[name]
                t0 = time.perf_counter()
                _lib.check(lib.rsvio_tracker_batch_process_frames(g["tb"]._h, C.addressof(g["tabs"][f][0]), C.byref(ms)))
                t1 = time.perf_counter()
                ws = None
                if g["single"] is not None:
                    t = g["single"]
                    t2 = time.perf_counter()
                    _lib.check(lib.rsvio_tracker_process_frame_device(
                        t._h, imgs[f, 0, 0].data_ptr(), imgs[f, 0, 1].data_ptr(), ptr(t._out_l), t.cap, C.byref(nl),
                        ptr(t._out_r), t.cap, C.byref(nr)))
                    ws = (time.perf_counter() - t2) * 1e3
                if k < a.warmup:
                    continue
                g["dev"].append(ms.value)
                g["wall"].append((t1 - t0) * 1e3)
                if ws is not None:
                    g["wall_single"].append(ws)
                g["feats"].append(float(np.mean([c.n_l for c in g["tabs"][f][0]])))
                if name != "off":
                    g["rej"].append(float(np.mean([t.gate_counts().n_rejected for t in g["ts"]])))
        for name in settings:
            g = legs[name]
            out[f"{name}/{n}"] = dict(device_ms=g["dev"], wall_ms=g["wall"], wall_single_ms=g["wall_single"],
                                      features_per_camera=float(np.median(g["feats"])),
                                      rejected_per_frame=float(np.median(g["rej"])) if g["rej"] else 0.0)
            g["tb"].close()
            for t in g["ts"] + ([g["single"]] if g["single"] else []):
                t.close()
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
                d = pooled.setdefault(f"{build}/{key}", dict(device_ms=[], wall_ms=[], wall_single_ms=[], info={}))
                for m in ("device_ms", "wall_ms", "wall_single_ms"):
                    d[m] += v[m]
                d["info"] = dict(features_per_camera=v["features_per_camera"], rejected_per_frame=v["rejected_per_frame"])
            print(f"round {rnd} {build} done", flush=True)
    if tmp:
        os.unlink(tmp.name)
    rows = []
    for key, d in pooled.items():
        build, setting, n = key.split("/")
        row = dict(build=build, setting=setting, n=int(n), **d["info"], device_ms=_stats(d["device_ms"]),
                   wall_ms=_stats(d["wall_ms"]))
        if d["wall_single_ms"]:
            row["wall_single_call_ms"] = _stats(d["wall_single_ms"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(shape=[W, H], levels=LEVELS, grid=GRID, focal=FOCAL, max_error=1.0 / FOCAL, rounds=a.rounds,
               reps_per_round=a.reps, rows=rows)
    by = {(r["build"], r["setting"], r["n"]): r for r in rows}
    if a.parent_lib:
        lvl = {}
        for n in (1, 64):
            for m in ("device_ms", "wall_ms"):
                p, t = by["parent", "off", n][m], by["tree", "off", n][m]
                lvl[f"n{n}_{m}"] = bool(p["p10"] <= t["p90"] and t["p10"] <= p["p90"])
        res["gate_off_level_with_parent"] = lvl
    res["gate_cost_device_us_per_frame"] = {
        f"{s}_n{n}": (by["tree", s, n]["device_ms"]["median"] - by["tree", "off", n]["device_ms"]["median"]) / n * 1e3
        for s in ("drop_right", "drop_both") for n in (1, 64)}
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tracker_stereo_gate_probe.json"))
    a = ap.parse_args()
    if a.reps < 30:
        ap.error("--reps must be at least 30")
    if a.worker:
        worker(a)
    else:
        driver(a)


if __name__ == "__main__":
    main()
