"""Batched motion tracking against n sequential single-stream calls.

For n in --n (default 1 8 64 256) streams, each with its own handle, its own 2,000-point map and a
config-4-sized frame (300 + 300 mapped features plus 40 + 40 without a map point; seeds differ per
stream), times
  (a) n sequential MotionTracker.track_motion calls (one launch and one host wait each), and
  (b) one MotionBatch.track_motion (one upload, one launch, one wait): wall time and device_ms,
and the same two for the robust path at --n-hyp hypotheses.  The *_abi legs make the same calls
on the C ABI with every argument marshalled beforehand (what a compiled caller pays: no numpy
conversion, no result objects), masks and hyp_count NULL on the robust path; batch_dev_abi is
batch_abi with every frame's lists already on the device (on_device = 1: no staging copy, the
upload is the argument table alone), so batch_abi - batch_dev_abi is the cost of staging and
uploading the lists.  Wall times are host clocks around calls that end in a stream synchronise;
every figure is the median of --reps repetitions after --warmup, the legs alternating inside each
repetition; p10 / p90 give the spread.  (b) is first checked to return (a)'s results bit for bit.

--single-only runs leg (a) alone: with RSVIO_LIB pointing at a library built from an earlier
commit it measures that commit's only way under the same caller.

usage: python tools/pnp_batch_probe.py [--n 1 8 64 256] [--reps 40] [--out profiles/x.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "rs-vio_amd")]

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

from rsvio import _lib  # noqa: E402
from rsvio import motion as M  # noqa: E402
from rsvio import synthetic as S  # noqa: E402


def _stats(x):
    x = np.asarray(x, np.float64)
    return dict(median=float(np.median(x)), p10=float(np.percentile(x, 10)), p90=float(np.percentile(x, 90)))


def _bits(r):
    return (r.status, r.iterations, r.n_observations, bool(r.is_keyframe), r.T_W_B.tobytes(),
            np.array([r.initial_cost, r.final_cost, r.translation_norm, r.rotation_norm]).tobytes())


def _abi_single(ts, fs, rc):
    """(plain, robust): the n single-stream C calls with prebuilt arguments."""
    lib = _lib.load()
    cfg, rcc = M.pnp_cfg(), rc.to_c()
    keep, plain, robust = [], [], []
    for t, m in zip(ts, fs):
        arrs = [np.ascontiguousarray(m.ids_l, np.uint64), np.ascontiguousarray(m.uv_l, np.float32),
                np.ascontiguousarray(m.ids_r, np.uint64), np.ascontiguousarray(m.uv_r, np.float32),
                np.ascontiguousarray(m.T_W_B_last_kf, np.float64), np.ascontiguousarray(m.T_C_B2, np.float64)]
        res, rres = _lib.MotionResult(), _lib.RobustMotionResult()
        keep.append((arrs, res, rres))
        p = [_lib.ptr(a) for a in arrs]
        head = (t._h, p[0], p[1], len(arrs[0]), p[2], p[3], len(arrs[2]), p[4], p[5], C.byref(cfg), C.byref(t.rule))
        plain.append(head + (C.byref(res),))
        robust.append(head + (C.byref(rcc), None, None, None, None, C.byref(rres)))

    def run_plain(_k=keep):
        for a in plain:
            _lib.check(lib.rsvio_track_motion(*a))

    def run_robust(_k=keep):
        for a in robust:
            _lib.check(lib.rsvio_track_motion_robust(*a))

    return run_plain, run_robust


def _device_frames(fs):
    """The frames with their lists as device tensors (ids as bytes at stride 8)."""
    import torch
    out = []
    for m in fs:
        d = {}
        for s in ("l", "r"):
            ids = np.ascontiguousarray(getattr(m, "ids_" + s), np.uint64)
            d["ids_" + s] = torch.from_numpy(ids.view(np.uint8).copy()).cuda()
            d["uv_" + s] = torch.from_numpy(np.ascontiguousarray(getattr(m, "uv_" + s), np.float32)).cuda()
        out.append(M.MotionFrame(d["ids_l"], d["uv_l"], d["ids_r"], d["uv_r"], m.T_W_B_last_kf, m.T_C_B2,
                                 on_device=True))
    torch.cuda.synchronize()
    return out


def _abi_batch(mb, bf, rc):
    lib = _lib.load()
    cfg, rcc = M.pnp_cfg(), rc.to_c()
    tab, keep = mb._frames(bf)
    res, rres = (_lib.MotionResult * mb.n)(), (_lib.RobustMotionResult * mb.n)()
    ms = C.c_double(0.0)
    pa = (mb._h, C.addressof(tab), C.byref(cfg), C.byref(mb.rule), C.addressof(res), C.byref(ms))
    ra = (mb._h, C.addressof(tab), C.byref(cfg), C.byref(mb.rule), C.byref(rcc), C.addressof(rres), C.byref(ms))

    def run_plain(_k=(tab, keep, res)):
        _lib.check(lib.rsvio_pnp_batch_track_motion(*pa))
        mb.device_ms = ms.value

    def run_robust(_k=(tab, keep, rres)):
        _lib.check(lib.rsvio_pnp_batch_track_motion_robust(*ra))
        mb.device_ms = ms.value

    return run_plain, run_robust


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n-hyp", type=int, default=256)
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 30:
        ap.error("--reps must be at least 30")
    batched = hasattr(M, "MotionBatch") and not a.single_only
    n_max = max(a.n)
    frames = [S.motion_frame(seed=100 + i) for i in range(n_max)]
    trackers = [M.MotionTracker() for _ in range(n_max)]
    for t, m in zip(trackers, frames):
        t.set_map(m.map_ids, m.map_pw)
    rc = M.RansacConfig(n_hyp=a.n_hyp, seed=1)
    rows = []
    for n in a.n:
        ts, fs = trackers[:n], frames[:n]

        def single():
            return [t.track_motion(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2)
                    for t, m in zip(ts, fs)]

        def single_robust():
            return [t.track_motion_robust(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2, rc)
                    for t, m in zip(ts, fs)]

        legs = {"single": single, "single_robust": single_robust}
        legs["single_abi"], legs["single_robust_abi"] = _abi_single(ts, fs, rc)
        mb = None
        if batched:
            mb = M.MotionBatch(ts)
            bf = [M.MotionFrame(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2) for m in fs]
            legs["batch"] = lambda: mb.track_motion(bf)
            legs["batch_robust"] = lambda: mb.track_motion_robust(bf, rc)
            legs["batch_abi"], legs["batch_robust_abi"] = _abi_batch(mb, bf, rc)
            legs["batch_dev_abi"], legs["batch_robust_dev_abi"] = _abi_batch(mb, _device_frames(fs), rc)
            assert [_bits(r) for r in mb.track_motion(_device_frames(fs))] == [_bits(r) for r in single()]
            assert [_bits(r) for r in legs["batch"]()] == [_bits(r) for r in single()]
            assert [_bits(r.motion) for r in legs["batch_robust"]()] == [_bits(r.motion) for r in single_robust()]
        wall = {k: [] for k in legs}
        dev = {k: [] for k in legs if k.startswith("batch")}
        kern = []
        for rep in range(a.warmup + a.reps):
            for k, fn in legs.items():
                t0 = time.perf_counter()
                out = fn()
                dt = (time.perf_counter() - t0) * 1e3
                if rep < a.warmup:
                    continue
                wall[k].append(dt)
                if k in dev:
                    dev[k].append(mb.device_ms)
                if k == "single":
                    kern.append(float(np.median([r.kernel_ms for r in out])))
        row = dict(n=n, n_hyp=a.n_hyp, reps=a.reps, label=a.label,
                   wall_ms={k: _stats(v) for k, v in wall.items()},
                   device_ms={k: _stats(v) for k, v in dev.items()},
                   single_kernel_ms=_stats(kern))
        if batched:
            for k in ("", "_abi"):
                row["gain" + k] = float(np.median(wall["single" + k]) / np.median(wall["batch" + k]))
                row["gain_robust" + k] = float(np.median(wall["single_robust" + k]) /
                                               np.median(wall["batch_robust" + k]))
            mb.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    for t in trackers:
        t.close()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
