"""Measurements for the device-side landmark triangulation (rsvio_ba_triangulate).

usage: python tools/triangulate_probe.py kernel      # device time per triangulate / check call (HIP events)
       python tools/triangulate_probe.py masked      # only masked triangulate calls: run it under
                                                     # rocprofv3 --kernel-trace --stats for the kernel's time
       python tools/triangulate_probe.py lm          # device time of one LM iteration of the config-3 solve
       python tools/triangulate_probe.py solve       # config-3 ray-start window: solve_ms / iterations, ray vs triangulated
       python tools/triangulate_probe.py estimator   # 72-frame stream, window 10: LM iterations and final-pose error

`lm` uses only entry points older than the triangulation, so RSVIO_LIB may point it at an earlier
build of the library for a same-session comparison.  Config 3: 10 keyframes, 2,000 landmarks,
24,000 observations; the ray start is the reference's depth-2.0 rule (sliding_window.rs:248-262).
"""
import dataclasses
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "rs-vio_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rsvio import _lib  # noqa: E402
from rsvio import synthetic as S  # noqa: E402
from rsvio.ba import BundleAdjuster, lm_cfg, se3_matrix  # noqa: E402


def ray_start(prob):
    T_B_C = [np.linalg.inv(np.asarray(T).reshape(4, 4)) for T in prob.T_C_B2]
    T_W_B = [np.linalg.inv(se3_matrix(p)) for p in prob.pose7]
    p = np.zeros((prob.n_lm, 3))
    seen = np.zeros(prob.n_lm, bool)
    for i in np.lexsort((prob.obs_cam, prob.obs_kf)):
        l = prob.obs_lm[i]
        if not seen[l]:
            seen[l] = True
            T = T_W_B[prob.obs_kf[i]] @ T_B_C[prob.obs_cam[i]]
            p[l] = T[:3, :3] @ np.array([prob.obs_uv[i, 0], prob.obs_uv[i, 1], 2.0]) + T[:3, 3]
    return p


def config3_ray():
    p = S.ba_problem(pose_noise=(0.005, 0.001))
    return dataclasses.replace(p, p_W=ray_start(p))


def adjuster(prob):
    ba = BundleAdjuster(max_keyframes=prob.n_kf, max_landmarks=prob.n_lm, max_observations=prob.n_obs)
    ba.set_problem_from(prob)
    return ba


def kernel(calls=200, warmup=20):
    from rsvio.ba import TRI_ALL_VIEWS, TRI_FIRST_STEREO, landmark_gate
    prob = config3_ray()
    ba = adjuster(prob)
    cs = _lib.CuStream(0)
    ba.set_stream(cs.ptr)
    ba.set_problem_from(prob)
    stream = torch.cuda.ExternalStream(cs.ptr)
    ones = np.ones(prob.n_lm, np.uint8)

    def timed(fn):
        for _ in range(warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(calls):
            fn()
        b.record(stream)
        b.synchronize()
        return 1e3 * a.elapsed_time(b) / calls

    for name, mode in (("all views", TRI_ALL_VIEWS), ("first stereo", TRI_FIRST_STEREO)):
        g = landmark_gate(mode)
        # (with a mask, back-to-back calls serialise: each waits until the previous kernel has read
        # the one staging buffer before refilling it -- a caller with one call per window never waits)
        print(f"triangulate, {name:12s}: {timed(lambda: ba.triangulate(None, g)):6.2f} us per call (no mask), "
              f"{timed(lambda: ba.triangulate(ones, g)):6.2f} us with a mask, serialised on its staging "
              f"({calls} back-to-back enqueue-only calls, HIP events)")
    pw, info, n = ba.triangulate(None, landmark_gate(TRI_ALL_VIEWS), want=True)
    print(f"accepted {n} of {prob.n_lm}; depths {info['min_depth'].min():.3f} .. {info['max_depth'].max():.3f} m")
    ba.run()
    # check_landmarks waits for its report: host wall time per call (kernel + 64 KB read-back)
    import time
    g = landmark_gate()
    for _ in range(warmup):
        ba.check_landmarks(g)
    t0 = time.perf_counter()
    for _ in range(calls):
        ba.check_landmarks(g)
    print(f"check_landmarks: {1e6 * (time.perf_counter() - t0) / calls:6.2f} us per call, host wall time "
          "(kernel, read-back of the report, stream wait)")
    ba.set_stream(None)
    ba.close()
    cs.close()


def masked(calls=200):
    from rsvio.ba import TRI_ALL_VIEWS, TRI_FIRST_STEREO, landmark_gate
    prob = config3_ray()
    ba = adjuster(prob)
    ones = np.ones(prob.n_lm, np.uint8)
    for mode in (TRI_ALL_VIEWS, TRI_FIRST_STEREO):
        g = landmark_gate(mode)
        for _ in range(calls):
            ba.triangulate(ones, g)
    print("accepted", ba.triangulate(ones, landmark_gate(TRI_ALL_VIEWS), want=True)[2])
    ba.close()


def lm(reps=15):
    """One LM iteration: the slope of the solve's device time (solve_ms) over the iteration cap."""
    prob = S.ba_problem()
    ba = adjuster(prob)
    caps, ms = (2, 3, 4, 5, 6), {}
    for c in caps:
        cfg = lm_cfg(max_iterations=c, cost_tolerance=0.0, parameter_tolerance=0.0)
        rs = []
        for _ in range(reps + 3):
            ba.set_problem_from(prob)
            rs.append(ba.run(cfg))
        assert all(r.iterations == c for r in rs), [r.iterations for r in rs]
        ms[c] = float(np.median([r.solve_ms for r in rs[3:]]))
    slope = np.polyfit(caps, [ms[c] for c in caps], 1)[0]
    print("config 3, solve_ms by iteration cap:", {c: round(v, 4) for c, v in ms.items()})
    print(f"one LM iteration: {1e3 * slope:.2f} us (least-squares slope over caps {caps}, median of {reps} solves each)")
    ba.close()


def solve(pairs=5):
    from rsvio.ba import TRI_ALL_VIEWS, TRI_FIRST_STEREO, landmark_gate
    prob = config3_ray()
    ba = adjuster(prob)
    for _ in range(3):
        ba.set_problem_from(prob)
        ba.run()
    for name, mode in (("all views", TRI_ALL_VIEWS), ("first stereo", TRI_FIRST_STEREO)):
        g = landmark_gate(mode)
        ray, tri = [], []
        for _ in range(pairs):
            ba.set_problem_from(prob)
            ray.append(ba.run())
            ba.set_problem_from(prob)
            ba.triangulate(None, g)
            tri.append(ba.run())
        for label, rs in (("ray start", ray), (f"triangulated ({name})", tri)):
            print(f"{label:28s}: solve_ms median {np.median([r.solve_ms for r in rs]):.4f} "
                  f"(all {[round(r.solve_ms, 4) for r in rs]}), iterations {rs[0].iterations}, "
                  f"initial cost {rs[0].initial_cost:.4g}, final cost {rs[0].final_cost:.6g}, status {rs[0].status}")
    ba.close()


def estimator():
    from rsvio.camera import Camera
    from rsvio.estimator import Estimator
    s, win = S.euroc_scene_stream(72), 10
    h, w = s.frames[0][0].shape
    cams = [Camera.opencv5(*p) for p in s.intrinsics]
    for mode in ("ray", "triangulate"):
        est = Estimator(w, h, cams, s.T_B_Cl, s.T_B_Cr, window=win, landmark_init=mode)
        iters = solves = sel = acc = 0
        outs = []
        for left, right in s.frames:
            r = est.process_frame(left, right)
            outs.append(r)
            if r.ba_status is not None:
                solves += 1
                iters += r.ba_iterations
                if est.window.last_triangulation:
                    sel += est.window.last_triangulation[0]
                    acc += est.window.last_triangulation[1]
        # (the project's convention, bench.py: translation of T_W_B against the stream's true pose)
        err = [float(np.linalg.norm(r.T_W_B[:3, 3] - np.asarray(T)[:3, 3])) for r, T in zip(outs, s.T_W_B)]
        print(f"{mode:12s}: {solves} full-window solves, {iters} LM iterations in total, pose error against the "
              f"stream's T_W_B: final {err[-1] * 1e3:.3f} mm, max {max(err) * 1e3:.3f} mm; "
              f"triangulated {acc} of {sel} selected")
        est.close()


if __name__ == "__main__":
    {"kernel": kernel, "masked": masked, "lm": lm, "solve": solve, "estimator": estimator}[sys.argv[1]]()
