"""Device time of robust motion tracking (rsvio_robust_motion_result.device_ms: the three launches
by HIP events) at n_hyp = 64, 256 and 1024 on synthetic.motion_frame's default input (600 joined
observations, 300 pairs, a 2,000-point map), beside the plain track_motion's kernel_ms from the
same process; medians of 200 calls after 20.  One process; its GPU step ends after `--limit`
seconds at the latest (SIGALRM's default action).  Prints one JSON object.
usage: python tools/robust_pnp_time.py [--limit 60] [--out FILE]"""
import argparse
import json
import signal
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "rs-vio_amd")]

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from rsvio import synthetic as S
    from rsvio.motion import MotionTracker, RansacConfig
    m = S.motion_frame(seed=3)
    signal.alarm(a.limit)  # the GPU step's time limit: an overrun ends the process
    mt = MotionTracker()
    mt.set_map(m.map_ids, m.map_pw)
    args = (m.ids_l, m.uv_l, m.ids_r, m.uv_r, m.T_W_B_last_kf, m.T_C_B2)

    def med(call, field):
        v = [getattr(call(), field) for _ in range(220)][20:]
        return 1e3 * float(np.median(v)), 1e3 * float(np.min(v))

    p = mt.track_motion(*args)
    plain = med(lambda: mt.track_motion(*args), "kernel_ms")
    out = {"input": "motion_frame(seed=3)", "n_observations": p.n_observations, "plain_iterations": p.iterations,
           "plain_kernel_us": round(plain[0], 2), "plain_kernel_us_min": round(plain[1], 2), "robust": []}
    for n_hyp in (64, 256, 1024):
        rc = RansacConfig(n_hyp=n_hyp)
        r = mt.track_motion_robust(*args, rc)
        dev = med(lambda: mt.track_motion_robust(*args, rc), "device_ms")
        refit = med(lambda: mt.track_motion_robust(*args, rc).motion, "kernel_ms")
        out["robust"].append({"n_hyp": n_hyp, "device_us": round(dev[0], 2), "device_us_min": round(dev[1], 2),
                              "refit_kernel_us": round(refit[0], 2), "ratio_to_plain": round(dev[0] / plain[0], 2),
                              "n_pairs": r.n_pairs, "best_hyp": r.best_hyp, "best_count": r.best_count,
                              "n_inliers": r.n_inliers, "iterations": r.motion.iterations,
                              "ransac_status": r.ransac_status})
    signal.alarm(0)
    mt.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
