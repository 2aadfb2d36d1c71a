"""Device time of rsvio_ba_covariance at config 3 (10 keyframes, 2,000 landmarks, 24,000
observations) and at config 5's shape (20 keyframes, 5,000 landmarks, 80,000 observations).

usage: python tools/covariance_probe.py [calls] [warmup]

After the default solve: warm-up, then `calls` calls of covariance(landmarks=True, full=True); the
median and minimum of device_ms (the call's own kernels by HIP events: the relinearisation, K4c,
ba_camera_covariance, ba_landmark_covariance) and of the call's wall time (which adds the copies
to the host and their waits).  Beside it the wall time of camera_step(0.0) on the same handle --
K4 + K4c + the camera solve, one synchronisation, 6 n_free doubles back -- whose work the
covariance call repeats before it inverts the factor; camera_step has no device timer of its own.
"""
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "rs-vio_amd")]

import numpy as np  # noqa: E402

from rsvio import synthetic as S  # noqa: E402
from rsvio.ba import COV_OK, BundleAdjuster  # noqa: E402


def measure(name, prob, calls, warmup):
    ba = BundleAdjuster(max_keyframes=21, max_landmarks=prob.n_lm, max_observations=prob.n_obs)
    ba.set_problem_from(prob)
    res = ba.run()
    dev, wall = [], []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        cov = ba.covariance(landmarks=True, full=True)
        t1 = time.perf_counter()
        assert cov.status == COV_OK
        if i >= warmup:
            dev.append(cov.device_ms)
            wall.append((t1 - t0) * 1e3)
    pose_only = []
    for i in range(warmup + calls):
        cov = ba.covariance()
        if i >= warmup:
            pose_only.append(cov.device_ms)
    step = []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        ba.camera_step(0.0)
        t1 = time.perf_counter()
        if i >= warmup:
            step.append((t1 - t0) * 1e3)
    ba.close()
    print(f"{name}: n_free {cov.n_free}, {prob.n_lm} landmarks, {prob.n_obs} observations, solve {res.iterations} it")
    print(f"  covariance device_ms   median {np.median(dev):.4f}  min {np.min(dev):.4f}  (all landmarks, full)")
    print(f"  covariance device_ms   median {np.median(pose_only):.4f}  min {np.min(pose_only):.4f}  (no landmark selected)")
    print(f"  covariance wall ms     median {np.median(wall):.4f}  min {np.min(wall):.4f}")
    print(f"  camera_step wall ms    median {np.median(step):.4f}  min {np.min(step):.4f}")


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    measure("config 3", S.ba_problem(), calls, warmup)
    measure("config 5 shape", S.ba_problem(n_kf=20, n_lm=5000, kf_per_lm=8, seed=55, init_seed=56), calls, warmup)


if __name__ == "__main__":
    main()
