#!/usr/bin/env python3
"""motion_covariance_probe.py [--reps 100] [--out profiles/motion_covariance_probe.json]

Time and accuracy of the motion covariance (rsvio_motion_covariance, rsvio_pnp_batch_covariance) on
one MI355X.  After a track_motion and a warm-up, `reps` calls each of
  * the default synthetic frame (600 factors) and the 4,096-feature frame: kernel_ms (the device
    wall clock inside the kernel) and the host wall time of the whole call;
  * a 64-slot batch of the default frame: device_ms (HIP events around the launch) and wall time;
  * track_motion on the default frame, in the same process, for scale.
Accuracy: the largest scaled error max |S - S_ref|_ij / sqrt(S_ref,ii S_ref,jj) against
tests/motion_covariance_reference.py over the parity frames of tests/test_motion_covariance_gpu.py,
at the tracked pose and at the last keyframe's.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "rs-vio_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))


def stats(x):
    x = np.asarray(x, np.float64)
    return dict(median=float(np.median(x)), min=float(x.min()), p90=float(np.percentile(x, 90)))


def timed(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    wall, out = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        out.append(r)
    return wall, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "motion_covariance_probe.json"))
    a = ap.parse_args()
    import motion_covariance_reference as R
    import rsvio
    from rsvio import synthetic as S
    from rsvio.motion import MotionBatch, MotionFrame, MotionTracker, pnp_cfg
    res = dict(device=rsvio.require_device(0), reps=a.reps, timing={}, accuracy={})
    mt = MotionTracker()
    for name, kw in (("default_600_factors", {}), ("capacity_4096_features", R.PARITY_FRAMES["capacity"])):
        m = S.motion_frame(**kw)
        lists = (m.ids_l, m.uv_l, m.ids_r, m.uv_r)
        mt.set_map(m.map_ids, m.map_pw)
        wall_t, r = timed(lambda: mt.track_motion(*lists, m.T_W_B_last_kf, m.T_C_B2), a.reps)
        T = r[-1].T_W_B
        wall_c, c = timed(lambda: mt.covariance(*lists, T, m.T_C_B2), a.reps)
        assert c[-1].status == 1
        res["timing"][name] = dict(n_observations=c[-1].n_observations,
                                   covariance_kernel_ms=stats([x.kernel_ms for x in c]),
                                   covariance_wall_ms=stats(wall_c),
                                   track_motion_kernel_ms=stats([x.kernel_ms for x in r]),
                                   track_motion_wall_ms=stats(wall_t), track_motion_iterations=r[-1].iterations)
    m = S.motion_frame()
    mt.set_map(m.map_ids, m.map_pw)
    T = mt.track_motion(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2).T_W_B
    mb = MotionBatch([mt] * 64)
    frames = [MotionFrame(m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2)] * 64
    Ts = np.stack([T] * 64)
    dev = []

    def batch():
        out = mb.covariance(frames, Ts)
        dev.append(mb.device_ms)
        return out
    wall_b, out = timed(batch, a.reps)
    res["timing"]["batch_64_slots"] = dict(device_ms=stats(dev[-a.reps:]), wall_ms=stats(wall_b),
                                           slot_kernel_ms=stats([x.kernel_ms for x in out[-1]]))
    mb.close()
    worst = 0.0
    for name, kw in R.PARITY_FRAMES.items():
        for delta in R.PARITY_DELTAS[name]:
            m = S.motion_frame(**kw)
            lists, map_ = (m.ids_l, m.uv_l, m.ids_r, m.uv_r), (m.map_ids, m.map_pw)
            mt.set_map(*map_)
            r = mt.track_motion(*lists, m.T_W_B_last_kf, m.T_C_B2, cfg=pnp_cfg(huber_delta=delta))
            for where, T in (("tracked", r.T_W_B), ("last_kf", m.T_W_B_last_kf)):
                H, Sg, cost, n, n_down = R.reference(lists, map_, T, m.T_C_B2, delta)
                c = mt.covariance(*lists, T, m.T_C_B2, delta)
                err = R.scaled_error(c.cov, Sg)
                worst = max(worst, err)
                res["accuracy"][f"{name}/delta={delta}/{where}"] = dict(
                    n=n, n_downweighted=n_down, kappa=float(np.linalg.cond(H)), scaled_error=err,
                    cost_rel=abs(c.cost - cost) / cost)
    res["largest_scaled_error"] = worst
    mt.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(dict(timing=res["timing"], largest_scaled_error=worst), indent=1))


if __name__ == "__main__":
    main()
